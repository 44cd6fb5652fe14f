"""Scripted constraint graphs for the island stage (islands.hip against oracle/oworld.hpp::update_islands), and the DEFINITION both are held to.

A scenario is a scene, a script {step: [action, ...]} applied before that step (steps count from 1), and a number of steps. Graphs are
built from two kinds of edge:
  * contact edges without points: weightless boxes (half extent 0.5, gravity 0) whose boxes lie within the creation margin of 0.02 m of
    each other without touching. An edge appears when a drifting body comes within 0.02 m and disappears once the gap exceeds the
    separation threshold (0.026 m). In sleeping scenarios bodies drift at 0.004 m/s or less, below the sleep thresholds;
  * null joints (JOINT_NULL: no rows, only a graph edge) between bodies that are far apart: any topology at any size. Adding or removing
    one is an edit: it forces the full relabel and wakes the islands it touches.
Actions (the same on the device world, the oracle and - where it offers them - the real engine):
  ("add_joints", [(a, b), ...])   null joints, indices continue the scene's
  ("remove_joints", [j, ...])     ("remove_bodies", [i, ...])     ("append", scene)     ("wake", [i, ...])
  ("set_asleep", [i, ...])        the listed bodies are put to sleep (sleeping tags, zero velocities)
  ("move_asleep", {i: position})  set_state with new positions - which wakes everything and restarts every timer - and the sleeping tags put back

The definition is written from the engine's description (island_manager.cpp: init_new_nodes_and_edges / merge_islands :117-350,
split_islands :352-522, put_islands_to_sleep :573-623, wake_up_island util/island_util.cpp:61-66), with islands named by their lowest
body index, in plain Python sets, floats and doubles:
  definition_labels   connected components over procedural, non-removed bodies; static and kinematic bodies do not connect;
  SleepDefinition     merge: the merged island continues with the timer of the biggest island it is made of, size = procedural bodies +
                      manifolds and joints that existed before this step, ties: the lowest old label; split: every part of an island
                      that fell apart starts its timer again; wake: a new manifold, or sleeping and awake bodies in one island; a wake
                      takes the sleeping tags off and leaves a running timer alone; removing a body or a joint wakes the islands it
                      touched, adding a joint those of its ends; an island whose lowest body is removed keeps its timer under the lowest
                      body left; decide: no body sleeping_disabled, none with |v|^2 > 0.005f^2 or |w|^2 > (pi/48)^2 in float: start the
                      timer at the previous step's stamp, sleep once stamp - since > 2.0 in double; else no timer.
Known deviations of oracle and device from the engine, documented in oracle/oworld.hpp: among islands of EQUAL size the engine keeps the
first in an ECS iteration order (here: the lowest old label), and its size also counts an island's non-procedural nodes. merge_tie, which
is nothing but the tie rule, stays out of the engine leg; no scenario puts a static body into an island that merges."""
import functools

import numpy as np

from edyn_amd import scenes

DYN, STA, KIN = scenes.KIND_DYNAMIC, scenes.KIND_STATIC, scenes.KIND_KINEMATIC
f32 = np.float32
G = 0.015            # a resting gap between neighbours: inside the creation margin, no contact
G0 = 0.0199          # the gap of an edge that is about to leave: it is destroyed after 0.0061 m of drift
V = 0.004            # drift speed in sleeping scenarios, below the linear sleep threshold of 0.005 m/s
P = 1.0 + G          # pitch of resting neighbours
LIN = f32(0.005)                                       # config/constants.hpp: island_linear_sleep_threshold
ANG = f32(3.1415926535897932384626433832795029) / f32(48.0)   # island_angular_sleep_threshold = pi / 48, in float as the sources compute it
TIME_TO_SLEEP = 2.0


def boxes(pos, vel=None, kind=None, nosleep=()):
    n = len(pos)
    s = scenes._empty(n)
    s["kind"][:] = DYN if kind is None else np.asarray(kind, np.int32)
    s["shape_type"][:] = scenes.SHAPE_BOX
    s["shape_param"][:, :3] = 0.5
    s["pos"][:] = np.asarray(pos, np.float32).reshape(n, 3)
    s["gravity"] = np.zeros((n, 3), np.float32)
    if vel is not None:
        s["linvel"][:] = np.asarray(vel, np.float32).reshape(n, 3)
    s["sleeping_disabled"] = np.zeros(n, np.uint8)
    s["sleeping_disabled"][list(nosleep)] = 1
    return s


def null_joint(a, b):
    return (scenes.JOINT_NULL, int(a), int(b), (0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0))


def permuted(scene, script, perm):
    """Body i of the scene becomes body perm[i]; joints and the script's indices follow."""
    perm = np.asarray(perm)
    inv = np.argsort(perm)
    out = {k: (np.ascontiguousarray(v[inv]) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    out["joints"] = [(j[0], int(perm[j[1]]), int(perm[j[2]])) + tuple(j[3:]) for j in scene.get("joints") or []]
    new_script = {}
    for step, acts in script.items():
        new_script[step] = []
        for a in acts:
            if a[0] == "add_joints":
                a = (a[0], [(int(perm[x]), int(perm[y])) for x, y in a[1]])
            elif a[0] == "move_asleep":
                a = (a[0], {int(perm[k]): v for k, v in a[1].items()})
            elif a[0] in ("remove_bodies", "wake", "set_asleep"):
                a = (a[0], [int(perm[x]) for x in a[1]])
            elif a[0] == "append":
                raise ValueError("appended bodies have no place in a permutation")
            new_script[step].append(a)
    return out, new_script


class Scenario:
    def __init__(self, name, scene, script=None, steps=2, sleeping=False, dt=1.0 / 60.0, claims=None, info=None):
        self.name, self.scene, self.script, self.steps, self.sleeping, self.dt = name, scene, script or {}, steps, sleeping, dt
        self.claims = claims      # claims(trace, scenario): what the scenario must contain, asserted on the ORACLE's trace
        self.engine = False       # part of the engine leg: decided in one place, all_scenarios()
        self.info = info or {}


# ------------------------------------------------------------------------------------------------ the definition
def pair_ends(keys):
    keys = np.asarray(keys, np.uint64)
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def definition_labels(n, kind, removed, pairs, joints):
    """Label of every body = the lowest index of its connected component; pairs: the world's pair keys, joints: live (a, b). Only
    procedural (dynamic, not removed) bodies connect; every other body is its own label."""
    proc = [(kind[i] == DYN) and not removed[i] for i in range(n)]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    a, b = pair_ends(pairs)
    edges = list(zip(a.tolist(), b.tolist())) + [(int(x), int(y)) for x, y in joints]
    for x, y in edges:
        if proc[x] and proc[y]:
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(i) for i in range(n)], np.uint32)


class SleepDefinition:
    """The sleep rules, carried from step to step: per-label timers, the previous labels, the previous pair set, the sleeping tags."""

    def __init__(self, kind, disabled, dt):
        self.kind = [int(k) for k in kind]
        self.removed = [False] * len(self.kind)
        self.disabled = [bool(d) for d in disabled]
        self.asleep = [False] * len(self.kind)
        self.labels = list(range(len(self.kind)))   # before the first update every body is alone
        self.prev_n = 0                               # bodies that had a label at the last update
        self.timers = {}                              # label -> stamp (absent: not running)
        self.pairs = set()
        self.joints = []                              # [a, b, alive]
        self.joints_seen = 0                          # joints that existed at the last update
        self.clock = 0.0                              # the stamp of the last update (the engine's m_last_time)
        self.dt = float(np.float32(dt))

    def proc(self, i):
        return self.kind[i] == DYN and not self.removed[i]

    def live_joints(self):
        return [(a, b) for a, b, alive in self.joints if alive]

    def _wake_island_of(self, i):
        if i < len(self.labels) and self.proc(i):
            l = self.labels[i]
            for k in range(len(self.labels)):
                if self.proc(k) and self.labels[k] == l:
                    self.asleep[k] = False

    # ---- edits
    def add_joints(self, ends):
        for a, b in ends:
            self.joints.append([a, b, True])
            self._wake_island_of(a); self._wake_island_of(b)

    def remove_joints(self, idx):
        for j in idx:
            if self.joints[j][2]:
                self.joints[j][2] = False
                self._wake_island_of(self.joints[j][0]); self._wake_island_of(self.joints[j][1])

    def wake(self, idx):
        for i in idx:
            self._wake_island_of(i)

    def set_asleep(self, idx):
        for i in idx:
            if self.proc(i) and not self.disabled[i]:
                self.asleep[i] = True

    def move_asleep(self, moves):   # set_state wakes every island and restarts every timer; the sleeping tags are put back afterwards
        self.timers = {}

    def append(self, kind, disabled):
        for k, d in zip(kind, disabled):
            self.kind.append(int(k)); self.removed.append(False); self.disabled.append(bool(d)); self.asleep.append(False)
            self.labels.append(len(self.labels))

    def remove_bodies(self, idx):
        for i in idx:
            if self.removed[i]:
                continue
            touched = [i]
            for key in self.pairs:
                a, b = int(key >> 32), int(key & 0xFFFFFFFF)
                if i in (a, b):
                    touched.append(b if a == i else a)
            for j in self.joints:
                if j[2] and i in (j[0], j[1]):
                    j[2] = False
                    touched.append(j[1] if j[0] == i else j[0])
            for t in touched:
                self._wake_island_of(t)
            self.pairs = {k for k in self.pairs if i not in (int(k >> 32), int(k & 0xFFFFFFFF))}
            was_proc, l = self.proc(i), self.labels[i] if i < len(self.labels) else i
            self.removed[i] = True; self.asleep[i] = False
            if was_proc and l == i:   # the island lives on under the lowest body that is left, timer included
                rest = [k for k in range(len(self.labels)) if k != i and self.proc(k) and self.labels[k] == i]
                t = self.timers.pop(i, None)
                if rest:
                    for k in rest:
                        self.labels[k] = rest[0]
                    if t is not None:
                        self.timers[rest[0]] = t
            if i < len(self.labels):
                self.labels[i] = i

    # ---- one island update
    def step(self, pairs, linvel, angvel):
        """pairs: the pair keys after this step's broadphase; velocities: the bodies' as the island update finds them (the state before
        the step). Returns (labels, asleep, timers by label)."""
        n = len(self.kind)
        pairs = set(int(k) for k in pairs)
        new_pairs = pairs - self.pairs
        labels = definition_labels(n, self.kind, self.removed, np.array(sorted(pairs), np.uint64), self.live_joints()).tolist()
        old = self.labels
        had = [i for i in range(min(self.prev_n, n)) if self.proc(i)]   # bodies that were in an island before this step

        def old_label_of_edge(a, b):
            x = a if self.proc(a) else b
            return old[x] if x < self.prev_n and self.proc(x) else None
        size = {}
        for i in had:
            size[old[i]] = size.get(old[i], 0) + 1
        for key in pairs & self.pairs:
            l = old_label_of_edge(int(key >> 32), int(key & 0xFFFFFFFF))
            if l is not None:
                size[l] = size.get(l, 0) + 1
        for a, b, alive in self.joints[:self.joints_seen]:
            if alive:
                l = old_label_of_edge(a, b)
                if l is not None:
                    size[l] = size.get(l, 0) + 1
        # merge: the biggest old island of every new island hands its timer on
        timers = {}
        best = {}
        for r in sorted(set(old[i] for i in had)):          # ascending: among equals the lowest old label stays
            if not (r < n and self.proc(r)):
                continue
            L = labels[r]
            if L not in best or size.get(r, 0) > size.get(best[L], 0):
                best[L] = r
        for L, r in best.items():
            if r in self.timers:
                timers[L] = self.timers[r]
        # split: every part of an old island that is now in more than one piece starts again
        parts = {}
        for i in had:
            parts.setdefault(old[i], set()).add(labels[i])
        for r, ls in parts.items():
            if len(ls) > 1:
                for L in ls:
                    timers.pop(L, None)
        # wake and decide
        lin2, ang2 = LIN * LIN, ANG * ANG
        members = {}
        for i in range(n):
            if self.proc(i):
                members.setdefault(labels[i], []).append(i)
        woken = set()
        for key in new_pairs:
            a, b = int(key >> 32), int(key & 0xFFFFFFFF)
            woken.add(labels[a] if self.proc(a) else labels[b])
        linvel = np.asarray(linvel, np.float32); angvel = np.asarray(angvel, np.float32)
        out_timers = {}
        for L, ms in members.items():
            sleeping = [self.asleep[i] for i in ms]
            wake = L in woken or (any(sleeping) and not all(sleeping))
            if all(sleeping) and not wake:
                continue
            for i in ms:
                self.asleep[i] = False
            quiet = not any(self.disabled[i] for i in ms)
            for i in ms:
                v, w = linvel[i], angvel[i]
                if (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) > lin2 or (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) > ang2:
                    quiet = False
            if quiet:
                t0 = timers.get(L)
                if t0 is None:
                    out_timers[L] = self.clock
                elif self.clock - t0 > TIME_TO_SLEEP:
                    for i in ms:
                        self.asleep[i] = True
                else:
                    out_timers[L] = t0
        self.timers, self.labels, self.prev_n, self.pairs, self.joints_seen = out_timers, labels, n, pairs, len(self.joints)
        self.clock = self.clock + self.dt
        return np.array(labels, np.uint32), np.array(self.asleep, bool), dict(out_timers)


def normalised_timers(labels, since, kind, removed):
    """{label: stamp or None} over the procedural, non-removed bodies that are their own label; None = not running (negative or NaN)."""
    out = {}
    for i in range(len(labels)):
        if kind[i] == DYN and not removed[i] and int(labels[i]) == i:
            out[i] = float(since[i]) if since[i] >= 0.0 else None
    return out


def definition_timers(labels, timers, kind, removed):
    return {i: timers.get(i) for i in range(len(labels)) if kind[i] == DYN and not removed[i] and int(labels[i]) == i}


# ------------------------------------------------------------------------------------------------ claims (on the oracle's trace)
def sleeps_at(trace, step, bodies=None):
    """The listed bodies (default: all procedural) are awake after step - 1 and asleep after `step`."""
    a0, a1 = trace[step - 2]["asleep"], trace[step - 1]["asleep"]
    idx = list(bodies) if bodies is not None else [i for i in range(len(a1)) if trace[step - 1]["proc"][i]]
    assert not a0[idx].any() and a1[idx].all(), (step, idx, a0.tolist(), a1.tolist())


def first_step(trace, pred):
    for t in trace:
        if pred(t):
            return t["step"]
    return None


def npairs(t):
    return len(t["pairs"])


# ------------------------------------------------------------------------------------------------ scenarios: certificate
RING_SLOTS = [(0, 0, 0), (1 + G0, 0.6, 0), (2 * (1 + G0), 0, 0), (1 + G0, -0.6, 0)]   # A - B - C - D - A; B leaves A when it drifts along +x


def ring4(rot, second_loss=False):
    """Four boxes in a cycle. Slot B drifts along +x at 0.004 m/s: its edge to A leaves after ~92 steps while its gap to C only narrows.
    rot: the body at slot k has index (k + rot) % 4, so the edge that leaves is (rot, rot + 1 mod 4). second_loss: C drifts as well, at
    0.0035 m/s, and leaves D ~13 steps later: the ring falls into {A, D} and {B, C}."""
    idx = [(k + rot) % 4 for k in range(4)]
    pos = np.zeros((4, 3)); vel = np.zeros((4, 3))
    for k in range(4):
        pos[idx[k]] = RING_SLOTS[k]
    vel[idx[1]] = (V, 0, 0)
    if second_loss:
        vel[idx[2]] = (0.0035, 0, 0)

    def claims(trace, sc):
        assert npairs(trace[0]) == 4 and trace[0]["num_islands"] == 1
        lost = first_step(trace, lambda t: npairs(t) == 3)
        assert lost is not None and 85 <= lost <= 100, lost
        sc.info["loss_step"] = lost
        if not second_loss:
            for t in trace:   # the island stays whole, its label and its timer do not change, and it falls asleep 2 s after the start
                assert t["num_islands"] == 1 and set(t["labels"].tolist()) == {0}
            assert all(t["timers"] == {0: 0.0} for t in trace[:120]), "the ring's timer does not run on through the loss"
            sleeps_at(trace, 121)
        else:
            split = first_step(trace, lambda t: npairs(t) == 2)
            assert split is not None and lost < split < 121 and trace[split - 2]["num_islands"] == 1 and trace[split - 1]["num_islands"] == 2
            stamp = trace[split - 1]["clock_before"]
            assert set(trace[split - 1]["timers"].values()) == {stamp}, "both parts start again at the split"
            sc.info["split_step"] = split
            sleeps_at(trace, split + 120)
    return Scenario(f"ring4-rot{rot}" + ("-split" if second_loss else ""), boxes(pos, vel), steps=(235 if second_loss else 124), sleeping=True,
                    claims=claims)


def two_paths():
    """Two boxes joined by a contact edge and by a null joint; the contact edge leaves (M goes to 0 with pm != 0): no split, the timer
    runs on."""
    s = boxes([(0, 0, 0), (1 + G0, 0, 0)], [(0, 0, 0), (V, 0, 0)])
    s["joints"] = [null_joint(0, 1)]

    def claims(trace, sc):
        lost = first_step(trace, lambda t: npairs(t) == 0)
        assert npairs(trace[0]) == 1 and lost is not None and lost < 121
        assert all(t["num_islands"] == 1 and t["timers"] == {0: 0.0} for t in trace[:120])
        sleeps_at(trace, 121)
    return Scenario("two_paths", s, steps=123, sleeping=True, claims=claims)


# ------------------------------------------------------------------------------------------------ scenarios: full relabel topologies
def _spread(n, pitch=3.0):
    k = np.arange(n)
    return np.stack([pitch * (k % 64), pitch * (k // 64), np.zeros(n)], 1)


def _with_contact_pair(pos):
    """Two more boxes that overlap each other, far from the rest: the world has a manifold, so the relabel's manifold kernels run."""
    far = np.array([[-10.0, -10.0, 0.0], [-10.0 + P, -10.0, 0.0]])
    return np.concatenate([pos, far])


def chain(n, order):
    """A path of n bodies joined by null joints, in ascending, descending or shuffled index order along the path; beside it three boxes
    in a row (indices n, n + 1, n + 2) of which the last drifts away at 0.06 m/s. Its edge - a certificate edge, the row is a tree -
    leaves after ~7 steps while the other manifold stays: that step relabels in full WITHOUT being forced, over the joints of the chain
    and a manifold, which is where the passes of EDYNHIP_CC_COMPRESS run and leave their path bit."""
    seq = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(n).permutation(n)}[order]
    row = np.array([[-10.0, -10.0, 0.0], [-10.0 + P, -10.0, 0.0], [-10.0 + P + 1 + G0, -10.0, 0.0]])
    vel = np.zeros((n + 3, 3)); vel[n + 2] = (0.06, 0, 0)
    s = boxes(np.concatenate([_spread(n), row]), vel)
    s["joints"] = [null_joint(seq[k], seq[k + 1]) for k in range(n - 1)]

    def claims(trace, sc):
        lost = first_step(trace, lambda t: npairs(t) == 1)
        assert npairs(trace[0]) == 2 and lost is not None and 3 < lost < sc.steps, lost
        for t in trace:
            assert (t["labels"][:n] == 0).all() and t["labels"][n:].tolist() == ([n, n, n] if t["step"] < lost else [n, n, n + 2])
            assert t["num_islands"] == (2 if t["step"] < lost else 3)
        sc.info["lost"] = lost
    return Scenario(f"chain-{n}-{order}", s, steps=10, claims=claims)


def star(hub_last):
    """1 024 singletons that all reach one hub - the highest index, or body 0 - and nobody else: every tree hooks under one root in the
    one launch of the first step's full relabel. Contact edges: a plate with 32 x 32 small boxes 0.015 m above it, 2 m apart (the device
    colours joints and allows a body 64 of them, so a hub of null joints is not a scene it accepts). As the highest index the hub owns
    all 1 024 pairs - a segment far beyond the 64 keys of the relabel's one-pass walk; as body 0 every other body owns one."""
    side = 32
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    small = np.stack([2.0 * i.ravel(), np.full(side * side, 0.1 + G + 0.5), 2.0 * j.ravel()], 1)
    plate = np.array([[side - 1.0, 0.0, side - 1.0]])
    n = side * side + 1
    hub = n - 1 if hub_last else 0
    s = boxes(np.concatenate([small, plate]) if hub_last else np.concatenate([plate, small]))
    s["shape_param"][hub, :3] = (side + 1.0, 0.1, side + 1.0)
    s["mass"][hub] = 1000.0

    def claims(trace, sc):
        assert all(npairs(t) == n - 1 and t["num_islands"] == 1 and (t["labels"] == 0).all() for t in trace)
    return Scenario(f"star-hub{'-last' if hub_last else '0'}", s, steps=2, claims=claims)


def comb():
    """64 chains of 16 joined at their far ends (the last body of every chain to the last body of the next)."""
    teeth, length = 64, 16
    n = teeth * length
    s = boxes(_with_contact_pair(_spread(n)))
    j = [null_joint(t * length + k, t * length + k + 1) for t in range(teeth) for k in range(length - 1)]
    j += [null_joint(t * length + length - 1, (t + 1) * length + length - 1) for t in range(teeth - 1)]
    s["joints"] = j

    def claims(trace, sc):
        assert all(t["num_islands"] == 2 and (t["labels"][:n] == 0).all() for t in trace)
    return Scenario("comb", s, steps=2, claims=claims)


COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)
STATICS = (0, 1, 4)


def counts(n, nstatic):
    """n dynamic bodies in islands of 3 interleaved by an index stride of about n / 3 (a wave holds ~21 distinct labels), one more
    island that has a body in every wave of 64, and nstatic static bodies: one at index 0, one at the highest index, the others in
    between; every static body is joined to two dynamic bodies of different islands and connects nothing."""
    total = n + nstatic
    static_at = sorted({0, total - 1, total // 3, (2 * total) // 3}) if nstatic == 4 else ([total - 1] if nstatic == 1 else [])
    if nstatic == 4 and len(static_at) < 4:
        static_at = sorted(set(static_at) | set(range(total)))[:4]
    kind = np.full(total, DYN)
    kind[static_at] = STA
    dyn = np.flatnonzero(kind == DYN)
    span = dyn[::64]                                   # one body of every wave: the spanning island
    rest = np.setdiff1d(dyn, span) if len(dyn) > 3 else dyn
    span = span if len(dyn) > 3 else dyn[:0]
    third = len(rest) // 3
    s = boxes(_spread(total), kind=kind)
    j = [null_joint(span[k], span[k + 1]) for k in range(len(span) - 1)]
    for k in range(third):
        j += [null_joint(rest[k + third], rest[k]), null_joint(rest[k + 2 * third], rest[k + third])]
    for q, st in enumerate(static_at):                # joints to a static body do not connect
        if len(dyn) >= 2:
            j += [null_joint(st, dyn[q % len(dyn)]), null_joint(dyn[(q + 1) % len(dyn)], st)]
    s["joints"] = j
    expect = (1 if len(span) else 0) + third + (len(rest) - 3 * third)

    def claims(trace, sc):
        assert all(t["num_islands"] == expect for t in trace), (trace[0]["num_islands"], expect)
    return Scenario(f"counts-{n}-statics{nstatic}", s, steps=2, claims=claims)


def bridge():
    """Two dynamic pairs that both touch one static box, and both touch one kinematic box; two more dynamic bodies each joined to one
    static body by null joints: separate islands throughout."""
    pos = [(0, 0, 0), (P, 0, 0),              # group 1: bodies 0, 1
           (2 * P, 0.5, 0),                   # 2: static, touches 1 and 3
           (3 * P, 0, 0), (4 * P, 0, 0),      # group 2: bodies 3, 4
           (2 * P, -0.55, 0),                 # 5: kinematic, touches 1 and 3 as well
           (20, 0, 0), (30, 0, 0), (25, 0, 0)]   # 6, 7 dynamic, 8 static: joints 6 - 8 - 7
    kind = [DYN, DYN, STA, DYN, DYN, KIN, DYN, DYN, STA]
    s = boxes(pos, kind=kind)
    s["joints"] = [null_joint(6, 8), null_joint(8, 7)]

    def claims(trace, sc):
        for t in trace:
            keys = set(t["pairs"].tolist())
            for a, b in ((2, 1), (3, 2), (5, 1), (5, 3)):
                assert ((max(a, b) << 32) | min(a, b)) in keys, (a, b)
            assert t["num_islands"] == 4 and t["labels"].tolist() == [0, 0, 2, 3, 3, 5, 6, 7, 8]
    return Scenario("bridge", s, steps=3, claims=claims)


def joints_only(sleeping):
    """Two islands of null joints and no manifold for ~20 steps (without sleeping this is the step's early return M == 0 && pm == 0), then
    a first contact appears between them: body 2 drifts towards body 0 along -x and comes within the margin."""
    v, t_in = (V if sleeping else 0.02), 20
    g_in = 0.02 + v * (t_in / 60.0)
    s = boxes([(0, 0, 0), (0, 5, 0), (1 + g_in, 0, 0), (10, 5, 0)], [(0, 0, 0), (0, 0, 0), (-v, 0, 0), (0, 0, 0)])
    s["joints"] = [null_joint(0, 1), null_joint(2, 3)]

    def claims(trace, sc):
        first = first_step(trace, lambda t: npairs(t) == 1)
        assert first is not None and first > 5 and all(npairs(t) == 0 for t in trace[:first - 1])
        assert trace[first - 2]["num_islands"] == 2 and trace[first - 1]["num_islands"] == 1
        sc.info["first_contact"] = first
    return Scenario("joints_only" + ("-sleeping" if sleeping else ""), s, steps=t_in + 10, sleeping=sleeping, claims=claims)


def joints_only_leaves(sleeping):
    """The same two islands of null joints, starting in contact; the contact leaves: pm != 0, M == 0, a real split."""
    v = V if sleeping else 0.02
    s = boxes([(0, 0, 0), (0, 5, 0), (1 + G0, 0, 0), (10, 5, 0)], [(0, 0, 0), (0, 0, 0), (v, 0, 0), (0, 0, 0)])
    s["joints"] = [null_joint(0, 1), null_joint(2, 3)]

    def claims(trace, sc):
        lost = first_step(trace, lambda t: npairs(t) == 0)
        assert npairs(trace[0]) == 1 and trace[0]["num_islands"] == 1 and lost is not None
        assert trace[lost - 1]["num_islands"] == 2 and trace[-1]["num_islands"] == 2 and lost + 2 < sc.steps
        sc.info["lost"] = lost
        if sleeping:
            assert set(trace[lost - 1]["timers"].values()) == {trace[lost - 1]["clock_before"]}
    return Scenario("joints_only-leaves" + ("-sleeping" if sleeping else ""), s, steps=(100 if sleeping else 25), sleeping=sleeping, claims=claims)


# ------------------------------------------------------------------------------------------------ scenarios: incremental hooks
RAIN_SIDE = 96


def rain(sleeping):
    """Two layers of 96 x 96 weightless boxes at a pitch of 1.5 m (boxes of one layer never meet); the upper layer drifts down at 0.06
    m/s and all 9 216 pairs are created in one step - more new edges than the 8 192 lanes of the two kernels that walk them. sleeping:
    the lower layer is put to sleep before the first step (set_asleep), so every one of the 9 216 new manifolds has to wake its island;
    the upper layer is too fast to run a timer."""
    k = RAIN_SIDE
    v = 0.06
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    low = np.stack([1.5 * i.ravel(), np.zeros(k * k), 1.5 * j.ravel()], 1)
    steps_in = 12
    gap0 = 0.02 + v * (steps_in / 60.0)
    up = low + np.array([0, 1.0 + gap0, 0])
    n = 2 * k * k
    vel = np.zeros((n, 3)); vel[k * k:] = (0, -v, 0)
    s = boxes(np.concatenate([low, up]), vel)
    script = {1: [("set_asleep", list(range(k * k)))]} if sleeping else {}

    def claims(trace, sc):
        arrival = first_step(trace, lambda t: npairs(t) > 0)
        assert arrival is not None and 2 <= arrival <= 30, arrival
        assert npairs(trace[arrival - 1]) == k * k > 8192, "the pairs do not all appear in one step"
        assert trace[arrival - 2]["num_islands"] == n and trace[arrival - 1]["num_islands"] == k * k
        assert (trace[arrival - 1]["labels"][k * k:] == np.arange(k * k)).all()
        if sleeping:
            before, after = trace[arrival - 2], trace[arrival - 1]
            assert before["asleep"][:k * k].all() and not before["asleep"][k * k:].any() and not after["asleep"].any()
            assert len(after["timers"]) == k * k and set(after["timers"].values()) == {None}
        sc.info["arrival"] = arrival
    return Scenario("rain" + ("-sleeping" if sleeping else ""), s, script, steps=steps_in + 4, sleeping=sleeping, claims=claims)


def funnel():
    """512 two-box islands along a line, and one long thin box that drifts down onto all of them: every island gains an edge to the
    same body in one step (one root contended by 512 hooks in the incremental mode)."""
    m = 512
    x = 2.5 * np.arange(m)
    a = np.stack([x, np.zeros(m), np.zeros(m)], 1)
    b = a + np.array([0, 0, P])
    v, steps_in = 0.06, 8
    gap0 = 0.02 + v * (steps_in / 60.0)
    bar = np.array([[x.mean(), 0.5 + 0.1 + gap0, 0.0]])
    pos = np.concatenate([bar, a, b])            # the bar is body 0: the root everybody hooks under
    vel = np.zeros((2 * m + 1, 3)); vel[0] = (0, -v, 0)
    s = boxes(pos, vel)
    s["shape_param"][0, :3] = (x.max() / 2 + 1.0, 0.1, 0.4)
    s["mass"][0] = 1000.0

    def claims(trace, sc):
        arrival = first_step(trace, lambda t: npairs(t) > m)
        assert arrival is not None and arrival > 1 and npairs(trace[arrival - 2]) == m and trace[arrival - 2]["num_islands"] == m + 1
        assert npairs(trace[arrival - 1]) == 2 * m and trace[arrival - 1]["num_islands"] == 1, (npairs(trace[arrival - 1]), trace[arrival - 1]["num_islands"])
        sc.info["arrival"] = arrival
    return Scenario("funnel", s, steps=steps_in + 4, claims=claims)


# ------------------------------------------------------------------------------------------------ scenarios: sleep-timer rules
def _three_way(name, X, Y, y_joints, untie=(30, 50), mirror=False, arrive=1.5, expect=None, steps=None):
    """Island X (boxes at the given offsets to the LEFT, the first at (-P, 0)), island Y (to the right, the first at (P, 0)) and the
    single box Z below the gap between them, drifting up at 0.004 m/s: after `arrive` seconds its box comes within the margin of X's and
    Y's first boxes in the same step, and the three islands merge. Until step untie[0] / untie[1] X / Y are tied by a null joint to a
    far-away sleeping_disabled anchor of their own, so they run no timer; the untying splits the anchor off and starts it. Z is timed from
    the first step. Indices: X, then Y, then Z, then the two anchors; mirror reverses them. expect(trace, info) adds the scenario's own
    claims; info has the index lists."""
    nx, ny = len(X), len(Y)
    pos = [(-P - x, y, 0) for x, y in X] + [(P + x, y, 0) for x, y in Y] + [(0, -(1 + 0.02 + V * arrive), 0), (-30, 40, 0), (30, 40, 0)]
    n = nx + ny + 3
    vel = np.zeros((n, 3)); vel[nx + ny] = (0, V, 0)
    s = boxes(pos, vel, nosleep=(n - 2, n - 1))
    ix, iy, z = list(range(nx)), list(range(nx, nx + ny)), nx + ny
    s["joints"] = [null_joint(n - 2, ix[-1]), null_joint(iy[-1], n - 1)] + [null_joint(iy[0], iy[1]) for _ in range(y_joints)]
    script = {untie[0]: [("remove_joints", [0])], untie[1]: [("remove_joints", [1])]}
    perm = np.arange(n)[::-1] if mirror else np.arange(n)
    s, script = permuted(s, script, perm)
    info = dict(X=[int(perm[i]) for i in ix], Y=[int(perm[i]) for i in iy], Z=int(perm[z]), anchors=[int(perm[n - 2]), int(perm[n - 1])], untie=untie)

    def claims(trace, sc):
        mx = len(set(trace[0]["pairs"].tolist()))
        merge = first_step(trace, lambda t: npairs(t) > mx)
        assert merge is not None and max(untie) < merge < 121, merge
        before, after = trace[merge - 2], trace[merge - 1]
        assert before["num_islands"] == 5 and after["num_islands"] == 3, (before["num_islands"], after["num_islands"])
        lx, ly, lz = (before["labels"][i] for i in (info["X"][0], info["Y"][0], info["Z"]))
        tx, ty, tz = (before["timers"][int(l)] for l in (lx, ly, lz))
        assert tz == 0.0 and tx == trace[untie[0] - 1]["clock_before"] and ty == trace[untie[1] - 1]["clock_before"], (tx, ty, tz)
        sc.info.update(info, merge_step=merge, tx=tx, ty=ty, tz=tz)
        merged = after["timers"][int(after["labels"][info["Z"]])]
        if expect is not None:
            expect(trace, sc, merged)
    return Scenario(name + ("-mirror" if mirror else ""), s, script, steps or 180, sleeping=True, claims=claims, info=info)


def merge3(mirror, y_joints=2):
    """Sizes (3 bodies + 2 manifolds) = 5, (2 bodies + 1 manifold + y_joints null joints) and 1 body, timers from steps 30, 50 and 1.
    With two joints the two big islands tie at 5 - only if joints count - and the lower old label's timer stays: X's, or Y's in the
    mirror; never Z's, the oldest. With three joints Y is the biggest whatever the labels."""
    def expect(trace, sc, merged):
        i = sc.info
        want = i["ty"] if (y_joints >= 3 or mirror) else i["tx"]
        assert merged == want and merged != i["tz"], (merged, i["tx"], i["ty"], i["tz"])
        sleeps_at(trace, (i["untie"][1] if want == i["ty"] else i["untie"][0]) + 120, i["X"] + i["Y"] + [i["Z"]])
    return _three_way(f"merge3-j{y_joints}", [(0, 0), (P, 0), (2 * P, 0)], [(0, 0), (P, 0)], y_joints, mirror=mirror, expect=expect, steps=175)


def merge_tie(mirror):
    """Two islands of two boxes and one manifold each, timed from steps 30 and 50 (and Z): the tie goes to the lowest old label."""
    def expect(trace, sc, merged):
        i = sc.info
        assert merged == (i["ty"] if mirror else i["tx"]), (merged, i["tx"], i["ty"])
    return _three_way("merge_tie", [(0, 0), (P, 0)], [(0, 0), (P, 0)], 0, mirror=mirror, expect=expect, steps=175)


def merge_edges_only(mirror=False):
    """Three boxes each; X is a row (2 manifolds), Y an L whose three boxes all reach each other (3 manifolds): Y is bigger by one
    persisting manifold, its timer - the youngest - stays."""
    def expect(trace, sc, merged):
        i = sc.info
        assert merged == i["ty"], (merged, i["tx"], i["ty"])
        sleeps_at(trace, i["untie"][1] + 120, i["X"] + i["Y"] + [i["Z"]])
    return _three_way("merge_edges_only", [(0, 0), (P, 0), (2 * P, 0)], [(0, 0), (P, 0), (0, P)], 0, mirror=mirror, expect=expect, steps=175)


def merge_then_split():
    """Null joints only, every body alone and quiet from the first step. Step 20: 0 - 1 joined (a merge of equals: timers equal anyway);
    step 21: the joint removed again (a split: both restart). Step 40, the same step on different islands: 2 - 3 are joined while 4 - 5,
    joined from the start, are cut."""
    s = boxes(_spread(6))
    s["joints"] = [null_joint(4, 5)]
    script = {20: [("add_joints", [(0, 1)])], 21: [("remove_joints", [1])], 40: [("add_joints", [(2, 3)]), ("remove_joints", [0])]}

    def claims(trace, sc):
        c = lambda k: trace[k - 1]["clock_before"]
        assert trace[18]["timers"] == {0: 0.0, 1: 0.0, 2: 0.0, 3: 0.0, 4: 0.0}
        assert trace[19]["timers"] == {0: 0.0, 2: 0.0, 3: 0.0, 4: 0.0}                      # merged: the timer runs on
        assert trace[20]["timers"] == {0: c(21), 1: c(21), 2: 0.0, 3: 0.0, 4: 0.0}           # split: both parts start again
        assert trace[39]["timers"] == {0: c(21), 1: c(21), 2: 0.0, 4: c(40), 5: c(40)}
        sleeps_at(trace, 121, [2, 3]); sleeps_at(trace, 141, [0, 1]); sleeps_at(trace, 160, [4, 5])
    return Scenario("merge_then_split", s, script, 162, sleeping=True, claims=claims)


def tombstone(middle=False):
    """Three boxes in a row, tied to an anchor until step 20 (timer from there), and Z, timed from step 1, drifting towards the row's
    free end. Step 40: the island's LOWEST index is removed. At the row's end (bodies 0 - 1 - 2): the rest stays whole, its name moves
    to body 1 and the timer runs on; when Z merges, the island of {1, 2} is the bigger one and the removed root is no candidate. In the
    middle (1 - 0 - 2): the island falls apart and both parts start again."""
    row = [(-3 * P, 0, 0), (-2 * P, 0, 0), (-P, 0, 0)] if not middle else [(-2 * P, 0, 0), (-P, 0, 0), (-3 * P, 0, 0)]
    # Z comes up beside the box at (-P, 0), as in _three_way
    pos = row + [(0, -(1 + 0.02 + V * 1.5), 0), (-30, 40, 0)]
    vel = np.zeros((5, 3)); vel[3] = (0, V, 0)
    s = boxes(pos, vel, nosleep=(4,))
    s["joints"] = [null_joint(4, 2)]
    script = {20: [("remove_joints", [0])], 40: [("remove_bodies", [0])]}

    def claims(trace, sc):
        c = lambda k: trace[k - 1]["clock_before"]
        assert trace[38]["timers"] == {0: c(20), 3: 0.0, 4: None} and trace[38]["labels"].tolist() == [0, 0, 0, 3, 4]
        merge = first_step(trace, lambda t: t["step"] > 40 and t["labels"][3] != 3)
        assert merge is not None and 80 < merge < 121, merge
        sc.info["merge_step"] = merge
        if not middle:
            assert trace[39]["labels"].tolist() == [0, 1, 1, 3, 4] and trace[39]["timers"] == {1: c(20), 3: 0.0, 4: None}
            assert trace[merge - 1]["timers"][1] == c(20)
            sleeps_at(trace, 140, [1, 2, 3])
        else:
            assert trace[39]["labels"].tolist() == [0, 1, 2, 3, 4] and trace[39]["timers"] == {1: c(40), 2: c(40), 3: 0.0, 4: None}
            assert trace[merge - 1]["timers"][1] == c(40)     # {1} and Z tie at one body each: the lower old label's timer
            sleeps_at(trace, 160, [1, 3])
    return Scenario("tombstone" + ("-middle" if middle else ""), s, script, 163, sleeping=True, claims=claims)


def append():
    """A timed island (two boxes untied from their anchor at step 100) and a sleeping one (two boxes, asleep from step 121). Before step
    150 two boxes are appended, one beside each: prev_n < n, the new bodies have no old label. The timed island takes its body in and
    keeps its timer; the sleeping island is woken by the new manifold and starts again."""
    s = boxes([(0, 0, 0), (P, 0, 0), (0, 10, 0), (P, 10, 0), (-30, 40, 0)], nosleep=(4,))
    s["joints"] = [null_joint(4, 1)]
    extra = boxes([(2 * P, 0, 0), (2 * P, 10, 0)])
    script = {100: [("remove_joints", [0])], 150: [("append", extra)]}

    def claims(trace, sc):
        c = lambda k: trace[k - 1]["clock_before"]
        assert trace[148]["asleep"].tolist() == [False, False, True, True, False] and trace[148]["timers"] == {0: c(100), 2: None, 4: None}
        assert trace[149]["labels"].tolist() == [0, 0, 2, 2, 4, 0, 2] and not trace[149]["asleep"].any()
        assert trace[149]["timers"] == {0: c(100), 2: c(150), 4: None}
        sleeps_at(trace, 220, [0, 1, 5]); sleeps_at(trace, 270, [2, 3, 6])
    return Scenario("append", s, script, 272, sleeping=True, claims=claims)


def nosleep():
    """Three quiet boxes in a row and one sleeping_disabled body tied to them by a null joint: no timer, no sleep. The joint is removed
    before step 150: the rest sleeps 2 s later, the disabled body never."""
    s = boxes([(0, 0, 0), (P, 0, 0), (2 * P, 0, 0), (0, 20, 0)], nosleep=(3,))
    s["joints"] = [null_joint(2, 3)]

    def claims(trace, sc):
        assert all(t["timers"] == {0: None} and not t["asleep"].any() for t in trace[:149])
        assert trace[149]["timers"] == {0: trace[149]["clock_before"], 3: None}
        sleeps_at(trace, 270, [0, 1, 2])
        assert not trace[-1]["asleep"][3]
    return Scenario("nosleep", s, {150: [("remove_joints", [0])]}, 272, sleeping=True, claims=claims)


def _diagonal_pair():
    """(x0, x1, y): float velocities (x, y, 0) with y = 0.004f whose float length_sqr is <= 0.005f^2 at x0 and > at x1 = the next float."""
    y = f32(0.004)
    x = f32(0.003)
    lin2 = LIN * LIN
    over = lambda x: (x * x + y * y + f32(0) * f32(0)) > lin2
    while over(x):
        x = np.nextafter(x, f32(0))
    while not over(np.nextafter(x, f32(1))):
        x = np.nextafter(x, f32(1))
    return x, np.nextafter(x, f32(1)), y


def threshold():
    """Free bodies at the thresholds, which are strict: |v| = 0.005f sleeps, the next float never; |w| = float(pi) / 48 sleeps, the next
    float never; a diagonal velocity whose float length_sqr is at most 0.005f^2 sleeps, one float further in x never."""
    x0, x1, y = _diagonal_pair()
    up = lambda a: np.nextafter(f32(a), f32(1))
    lv = [(LIN, 0, 0), (up(LIN), 0, 0), (0, 0, 0), (0, 0, 0), (x0, y, 0), (x1, y, 0), (0, 0, LIN), (0, up(LIN), 0)]
    s = boxes(_spread(8, 10.0), lv)
    s["angvel"][2] = (0, ANG, 0); s["angvel"][3] = (0, up(ANG), 0)
    quiet, fast = [0, 2, 4, 6], [1, 3, 5, 7]

    def claims(trace, sc):
        lin2 = LIN * LIN
        assert (x0 * x0 + y * y) <= lin2 < (x1 * x1 + y * y) and up(LIN) * up(LIN) > lin2 and up(ANG) * up(ANG) > ANG * ANG
        sleeps_at(trace, 121, quiet)
        assert not any(t["asleep"][fast].any() for t in trace) and all(t["timers"][i] is None for t in trace for i in fast)
    return Scenario("threshold", s, steps=124, sleeping=True, claims=claims)


def sleep_step(dt):
    """The first step at which a body that is quiet from the start sleeps: the double clock advances by float(dt) per step, the timer
    starts at the stamp the first update sees (0), and the comparison is a strict > 2.0."""
    clock, since, d = 0.0, None, float(np.float32(dt))
    for step in range(1, 10000):
        if since is None:
            since = clock
        elif clock - since > TIME_TO_SLEEP:
            return step
        clock = clock + d
    raise AssertionError


def two_seconds(dt, tag):
    want = sleep_step(dt)

    def claims(trace, sc):
        sleeps_at(trace, want, [0])
    return Scenario(f"two_seconds-{tag}", boxes([(0, 0, 0)]), steps=want + 1, sleeping=True, dt=dt, claims=claims, info=dict(sleep_step=want))


def nonprocedural_meets_sleepers(kind):
    """A sleeping island of two boxes (asleep from step 121); before step 150 a static or a kinematic box is appended 0.015 m beside it,
    inside the margin (a kinematic body is not integrated, so it cannot drift there: it is placed, like the static one). Only awake
    procedural bodies look for pairs (broadphase.cpp:183-192), so no manifold is made and the island sleeps on: the engine leg holds the
    oracle to that. Body 2, adrift above the threshold, keeps the world from being asleep as a whole."""
    s = boxes([(0, 0, 0), (P, 0, 0), (20, 0, 0)], [(0, 0, 0), (0, 0, 0), (0.01, 0, 0)])
    script = {150: [("append", boxes([(-P, 0, 0)], kind=[kind]))]}

    def claims(trace, sc):
        sleeps_at(trace, 121, [0, 1])
        assert all(npairs(t) == 1 and t["asleep"][:2].all() and not t["asleep"][2] for t in trace[120:])
        # on the oracle's state at the end: the appended box's face is inside the margin of body 0's, and not touching
        assert 0.0 < float(trace[-1]["pos"][0][0]) - float(trace[-1]["pos"][3][0]) - 1.0 < 0.02
    return Scenario("static_meets_sleepers" if kind == STA else "kinematic_meets_sleepers", s, script, 175, sleeping=True, claims=claims)


def sleeping_owner(variant):
    """Boxes 1 and 2 fall asleep at step 121 (one manifold, kept by its sleeping owner, body 2). An awake box passes body 2 at 2 m/s with
    its side 0.015 m from body 2's, inside the margin from step ~132 to ~193, and leaves again.
      filtered  the passer-by is body 0 and the collision filter keeps it apart from body 2: no manifold, nobody wakes, and the sleeping
                owner's kept manifold is counted once - never a full relabel after the first step;
      low       body 0, unfiltered: an awake body reaches a sleeping owner with a higher index; the manifold wakes the island;
      high      the passer-by is body 3: it owns the new manifold itself;
      moved     nobody passes; before step 140 the sleeping body 2 is set 30 m away (set_state, then the sleeping tags put back): the
                kept manifold stays - separated manifolds of sleeping bodies are not destroyed - and so does the island."""
    y0 = -(1.02 + 2.0 * (131 / 60.0))
    passer = (2 * P, y0, 0) if variant != "moved" else (50, y0, 0)
    pos, vel = [(0, 0, 0), (P, 0, 0)], [(0, 0, 0), (0, 0, 0)]
    if variant == "high":
        pos, vel, ip, sl = pos + [passer], vel + [(0, 2.0, 0)], 2, [0, 1]
    else:
        pos, vel, ip, sl = [passer] + pos, [(0, 2.0, 0)] + vel, 0, [1, 2]
    s = boxes(pos, vel)
    script = {}
    if variant == "filtered":
        s["group"][ip] = np.uint64(2)
        s["mask"][sl[1]] = np.uint64(2**64 - 1 - 2)
    if variant == "moved":
        script = {140: [("move_asleep", {sl[1]: (30.0, 0.0, 0.0)})]}
    key = (max(ip, sl[1]) << 32) | min(ip, sl[1])

    def claims(trace, sc):
        sleeps_at(trace, 121, sl)
        met = [t["step"] for t in trace if key in set(t["pairs"].tolist())]
        if variant in ("filtered", "moved"):
            assert not met and all(npairs(t) == 1 and t["asleep"][sl].all() and t["num_islands"] == 2 for t in trace[120:])
        else:
            assert met and 125 <= met[0] <= 140 and met[-1] < sc.steps - 2 and met == list(range(met[0], met[-1] + 1)), met
            woke, gone = trace[met[0] - 1], trace[met[-1]]
            assert not woke["asleep"].any() and woke["num_islands"] == 1 and woke["timers"] == {0: None}
            assert gone["num_islands"] == 2 and gone["timers"][sl[0]] == gone["clock_before"], "the parts start again when the passer-by leaves"
            sc.info.update(met=met[0], left=met[-1] + 1)
    return Scenario(f"sleeping_owner-{variant}", s, script, 200, sleeping=True, claims=claims)


def crowded_owner(k):
    """bplayouts.owner_k(k): one big sphere, created last, with exactly k small spheres inside its box (k = 63, 64, 65: the 64 keys of an
    owner's segment - beyond them the relabel's two-pass walk; 127, 128, 129: the candidate list), 20 singletons far away. One partner
    drifts out of the box at 1.5 m/s and is alone after ~10 steps."""
    import bplayouts
    s = bplayouts.owner_k(k)
    n = len(s["kind"])
    inside = [i for i in range(n - 1) if 1.85 < s["pos"][i][0] < 3]
    out = inside[len(inside) // 2]
    s["linvel"][out] = (1.5, 0, 0)

    def claims(trace, sc):
        first = min(i for i in range(n - 1) if abs(s["pos"][i]).max() < 3)
        assert npairs(trace[0]) == k and trace[0]["num_islands"] == 21 and trace[0]["labels"][n - 1] == first
        left = first_step(trace, lambda t: npairs(t) == k - 1)
        assert left is not None and 3 < left < sc.steps and trace[-1]["num_islands"] == 22 and trace[-1]["labels"][out] == out
        sc.info["left"] = left
    return Scenario(f"crowded_owner-{k}", s, steps=14, claims=claims)


def joint_wakes():
    """Two sleeping singletons are joined by a null joint before step 200 (a new edge wakes what it joins), a wake_up_entity on a timed
    island at step 60 changes nothing, and a joint removed from an island that stays connected through a contact leaves its timer alone."""
    s = boxes([(0, 0, 0), (10, 0, 0), (0, 10, 0), (P, 10, 0), (0, 20, 0)])
    s["joints"] = [null_joint(2, 3)]
    script = {60: [("wake", [4]), ("remove_joints", [0])], 200: [("add_joints", [(0, 1)])]}

    def claims(trace, sc):
        sleeps_at(trace, 121)
        assert trace[199]["asleep"].tolist() == [False, False, True, True, True] and trace[199]["labels"].tolist() == [0, 0, 2, 2, 4]
        assert trace[199]["timers"][0] == trace[199]["clock_before"]
        sleeps_at(trace, 320, [0, 1])
    return Scenario("joint_wakes", s, script, 322, sleeping=True, claims=claims)


def joint_wakes_engine():
    """joint_wakes without the wake_up_entity (the engine binding has none)."""
    sc = joint_wakes()
    sc.name = "joint_wakes-engine"
    sc.script = {60: [("remove_joints", [0])], 200: [("add_joints", [(0, 1)])]}
    return sc


@functools.lru_cache(maxsize=None)
def all_scenarios():
    out = [ring4(r) for r in range(4)] + [ring4(0, True), ring4(2, True), two_paths()]
    out += [chain(n, o) for n in (300, 1025) for o in ("ascending", "descending", "shuffled")]
    out += [star(True), star(False), comb()]
    out += [counts(n, ns) for ns in STATICS for n in COUNTS]
    out += [bridge(), joints_only(False), joints_only(True), joints_only_leaves(False), joints_only_leaves(True)]
    out += [rain(False), rain(True), funnel()]
    out += [merge3(False), merge3(True), merge3(False, 3), merge3(True, 3), merge_tie(False), merge_tie(True), merge_edges_only(False),
            merge_edges_only(True), merge_then_split(), tombstone(False), tombstone(True), append(), nosleep(), threshold(),
            two_seconds(1.0 / 60.0, "60"), two_seconds(1.0 / 64.0, "64"), two_seconds(0.25, "4"),
            nonprocedural_meets_sleepers(KIN), nonprocedural_meets_sleepers(STA), joint_wakes(), joint_wakes_engine()]
    out += [sleeping_owner(v) for v in ("filtered", "low", "high", "moved")] + [crowded_owner(k) for k in (63, 64, 65, 127, 128, 129)]
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    # The engine leg runs everything but: merge_tie (it rests on the tie rule, a documented deviation), joint_wakes and
    # sleeping_owner-moved (wake_up_entity and the sleeping tags are not in the engine binding; joint_wakes-engine is the former without
    # the wake) and rain (7 s a run on the engine; its rules are those of funnel).
    for s in out:
        s.engine = not s.name.startswith(("merge_tie", "rain", "sleeping_owner-moved")) and s.name != "joint_wakes"
    return out


def by_name(name):
    return next(s for s in all_scenarios() if s.name == name)
