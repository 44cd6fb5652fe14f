"""Island labels, relabel modes and sleep timers on SCRIPTED graphs: the device's island stage (islands.hip) against the oracle's, the
oracle's against the real engine's, and the oracle's against a plain-Python statement of the definition (tests/islandgraphs.py).

The oracle rebuilds the components from scratch in every step; the device keeps labels incrementally, chooses per step between skipping,
hooking only the new manifolds (CC_INCREMENTAL) and a full lock-free relabel (CC_FULL) from a count of certificate manifolds, and alone
has to carry timers through merges by a size rule. The ordinary scenes never show it what islandgraphs.py builds: cycles that lose a
certificate or a non-certificate edge, three-way merges and size ties, joints as edges of the size count, islands that meet only in a
static or kinematic body, long chains in shuffled index order, a thousand trees hooking under one root, more new edges in a step than
the hooking kernels have lanes, removed roots, bodies appended to a sleeping world, body counts at every wave and block boundary, and
the strict thresholds of the sleep decision.

Three legs:
  * oracle against the definition (CPU): every scenario, every step - labels, island count, sleeping flags, normalised timers;
  * oracle against the real engine (CPU; skipped where oracle/_ref was not built), in lock-step as tests/test_reference_engine.py
    does it: state, pair keys, sleeping flags, island partition and island count at every step. Left out: merge_tie, which is
    nothing but the tie rule (among islands of equal size the engine keeps the first in an ECS iteration order; oracle/oworld.hpp
    documents that deviation and the other one, non-procedural nodes in an island's size); joint_wakes and sleeping_owner-moved,
    which use wake_up_entity and the sleeping tags that the engine binding does not offer; rain, for its size;
  * device against oracle (gpu): every scenario, every step - labels of the procedural bodies, island count, sleeping flags, normalised
    timers, pair keys, the state at the end; the device's labels also against the definition over the device's own pair set; and the
    relabel modes from World.debug_relabel_steps().
What a scenario must contain (a merge of three islands at step k with these timers, 9 216 pairs in one step) is asserted on the oracle's
trace, never on the device's; only the modes, which exist on the device alone, are asserted there. No tolerance anywhere.

Found by these scenarios and fixed in oracle and device (each confirmed against the engine first):
  * waking an island - a removed joint or body, wake_up_entity - restarted its sleep timer; the engine's wake_up_island only takes the
    sleeping tags off, so an island that stays connected sleeps 2 s after it became quiet, not 2 s after the edit;
  * an island whose lowest-index body was removed lost its timer with its name, whole or not;
  * a joint added between sleeping islands left them asleep; in the engine a new edge wakes what it joins;
  * joints created since the last update counted towards the size of the island of their first body in that step's merge."""
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from oracle import binding as ob
import islandgraphs as ig

SCENARIOS = ig.all_scenarios()
NAMES = [s.name for s in SCENARIOS]
ENGINE = [s.name for s in SCENARIOS if s.engine]


# ------------------------------------------------------------------------------------------------ the three kinds of world
class _Side:
    """A world under one interface: the scenario's actions, one step, and what the legs compare."""

    def apply(self, act):
        getattr(self, "do_" + act[0])(*act[1:])


class OracleSide(_Side):
    def __init__(self, sc, order=ob.ORDER_COLOURED):
        self.w = ob.World(dt=sc.dt, vel_iters=10, pos_iters=3, order=order)
        self.w.add_bodies(sc.scene)
        self._flags(sc.scene, 0)
        if sc.sleeping:
            self.w.set_sleeping(True)

    def _flags(self, scene, first):
        for i in np.flatnonzero(scene.get("sleeping_disabled", np.zeros(0))):
            self.w.set_sleeping_disabled(first + int(i), True)

    def do_add_joints(self, ends):
        for a, b in ends:
            self.w.add_joint(*ig.null_joint(a, b))

    def do_remove_joints(self, idx):
        for j in idx:
            self.w.remove_joint(j)

    def do_remove_bodies(self, idx):
        for i in idx:
            self.w.remove_body(i)

    def do_append(self, scene):
        first = self.w.num_bodies
        self.w.add_bodies(scene)
        self._flags(scene, first)

    def do_wake(self, idx):
        self.w.wake_bodies(idx)

    def do_set_asleep(self, idx):
        flags = self.w.get_asleep()
        flags[idx] = True
        self.w.set_asleep(flags)

    def do_move_asleep(self, moves):
        flags = self.w.get_asleep()
        pos, orn, lv, av = self.w.get_state()
        for i, p in moves.items():
            pos[i] = p
        self.w.set_state(pos, orn, lv, av)
        self.wake_all_like_set_state()
        self.w.set_asleep(flags)

    def wake_all_like_set_state(self):   # the device's set_state wakes every island (edynhip.h); the oracle's only writes the state
        self.w.wake_all()

    def step(self):
        self.w.step(1)

    def labels(self):
        return self.w.get_derived()[2]

    def num_islands(self):
        return self.w.get_stats()["num_islands"]


class DeviceSide(OracleSide):
    def __init__(self, sc):
        self.w = edyn_amd.World(edyn_amd.init_config(fixed_dt=sc.dt, num_solver_velocity_iterations=10, num_solver_position_iterations=3,
                                                     sleeping=sc.sleeping, max_manifolds=max(1 << 14, 2 * len(sc.scene["kind"])),
                                                     max_bodies=len(sc.scene["kind"]) + 8, max_joints=len(sc.scene.get("joints") or []) + 8))
        self.w.set_scene(sc.scene)

    def do_add_joints(self, ends):
        self.w.add_joints([ig.null_joint(a, b) for a, b in ends])

    def do_remove_joints(self, idx):
        self.w.remove_joints(idx)

    def do_remove_bodies(self, idx):
        self.w.remove_bodies(idx)

    def do_append(self, scene):
        self.w.add_scene(scene)

    def wake_all_like_set_state(self):
        pass

    def step(self):
        self.w.step_simulation(1)


class EngineSide(_Side):
    def __init__(self, sc):
        self.w = ob.RefWorld(dt=sc.dt, vel_iters=10, pos_iters=3)
        self.sleeping = sc.sleeping
        self._add(sc.scene)
        for j in sc.scene.get("joints") or []:
            self.w.add_joint(*j)

    def _add(self, scene):   # body by body: the engine binding takes sleeping_disabled per call
        dis = scene.get("sleeping_disabled", np.zeros(len(scene["kind"]), np.uint8))
        for i in range(len(scene["kind"])):
            self.w.add_bodies(scenes.subset(scene, np.array([i])), sleeping_disabled=bool(dis[i]) or not self.sleeping)

    def do_add_joints(self, ends):
        for a, b in ends:
            self.w.add_joint(*ig.null_joint(a, b))

    def do_remove_joints(self, idx):
        for j in idx:
            self.w.remove_joint(j)

    def do_remove_bodies(self, idx):
        for i in idx:
            self.w.remove_body(i)

    def do_append(self, scene):
        self._add(scene)


class _Book:
    """The scene's description as the script changes it: kinds, removed bodies, live joints, sleeping_disabled (for the definition and the
    masks of the comparisons)."""

    def __init__(self, sc):
        self.kind = [int(k) for k in sc.scene["kind"]]
        self.removed = [False] * len(self.kind)
        self.disabled = [bool(d) for d in sc.scene.get("sleeping_disabled", np.zeros(len(self.kind)))]

    def apply(self, act):
        if act[0] == "remove_bodies":
            for i in act[1]:
                self.removed[i] = True
        elif act[0] == "append":
            self.kind += [int(k) for k in act[1]["kind"]]
            self.removed += [False] * len(act[1]["kind"])
            self.disabled += [bool(d) for d in act[1].get("sleeping_disabled", np.zeros(len(act[1]["kind"])))]

    def proc(self):
        return np.array([k == ig.DYN and not r for k, r in zip(self.kind, self.removed)], bool)


def _observe(side, book, sleeping):
    proc = book.proc()
    out = dict(labels=side.labels().copy(), num_islands=side.num_islands(), pairs=side.w.get_pairs().copy(), proc=proc,
               asleep=side.w.get_asleep().copy() if sleeping else np.zeros(len(proc), bool), timers={})
    if sleeping:
        lab, since, clock = side.w.get_sleep_timers()
        assert np.array_equal(lab[proc], out["labels"][proc])
        out["timers"] = ig.normalised_timers(lab, since, book.kind, book.removed)
        out["clock"] = clock
    return out


# ------------------------------------------------------------------------------------------------ the oracle's trace, and the definition beside it
@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    """Every step of the scenario on the oracle - computed once, shared by the legs, never changed - with the definition run beside it
    on the oracle's pair sets and velocities: (trace, definition's trace, the oracle's state at the end)."""
    sc = ig.by_name(name)
    o, book = OracleSide(sc), _Book(sc)
    d = ig.SleepDefinition(book.kind, book.disabled, sc.dt)
    d.add_joints([(j[1], j[2]) for j in sc.scene.get("joints") or []])
    trace, dtrace = [], []
    clock = 0.0
    for step in range(1, sc.steps + 1):
        for act in sc.script.get(step, []):
            o.apply(act); book.apply(act)
            if act[0] == "append":
                d.append(act[1]["kind"], act[1].get("sleeping_disabled", np.zeros(len(act[1]["kind"]))))
            else:
                getattr(d, act[0])(act[1])
        _, _, lv, av = o.w.get_state()
        o.step()
        t = _observe(o, book, sc.sleeping)
        t.update(step=step, clock_before=clock)
        clock = clock + float(np.float32(sc.dt))
        if sc.sleeping:
            assert t["clock"] == clock, (name, step, "the oracle's clock is not the sum of float(dt)")
        if step == sc.steps:
            t["pos"] = o.w.get_state()[0].copy()   # the oracle's positions at the end, for claims about where a body got to
        trace.append(t)
        if sc.sleeping:
            dl, da, dt_ = d.step(t["pairs"], lv, av)
            dtrace.append(dict(labels=dl, asleep=da, timers=ig.definition_timers(dl, dt_, book.kind, book.removed)))
        else:
            dl = ig.definition_labels(len(book.kind), book.kind, book.removed, t["pairs"], _live_joints(sc, step))
            dtrace.append(dict(labels=dl, asleep=t["asleep"], timers={}))
    return trace, dtrace, o.w.get_state()


def _live_joints(sc, upto_step):
    joints = [[j[1], j[2], True] for j in sc.scene.get("joints") or []]
    removed = set()
    for step in sorted(sc.script):
        if step > upto_step:
            break
        for act in sc.script[step]:
            if act[0] == "add_joints":
                joints += [[a, b, True] for a, b in act[1]]
            elif act[0] == "remove_joints":
                for j in act[1]:
                    joints[j][2] = False
            elif act[0] == "remove_bodies":
                removed |= set(act[1])
    return [(a, b) for a, b, alive in joints if alive and a not in removed and b not in removed]


def scenario_with_info(name):
    """The scenario after its claims ran on the oracle's trace: they also note the steps of its events in sc.info."""
    sc = ig.by_name(name)
    if sc.claims and not sc.info.get("claimed"):
        sc.claims(oracle_trace(name)[0], sc)
        sc.info["claimed"] = True
    return sc


# ------------------------------------------------------------------------------------------------ leg A: oracle against the definition
@pytest.mark.parametrize("name", NAMES)
def test_oracle_islands_match_the_definition(name):
    """Labels, island count, sleeping flags and timers of the oracle at every step equal the definition's over the oracle's pair sets;
    and the scenario contains what it claims."""
    sc = ig.by_name(name)
    trace, dtrace, _ = oracle_trace(name)
    for t, d in zip(trace, dtrace):
        p = t["proc"]
        assert np.array_equal(t["labels"][p], d["labels"][p]), (name, t["step"], "labels")
        assert t["num_islands"] == int((d["labels"][p] == np.flatnonzero(p)).sum()), (name, t["step"], "island count")
        if sc.sleeping:
            assert np.array_equal(t["asleep"][p], d["asleep"][p]), (name, t["step"], "sleeping flags", t["asleep"].tolist(), d["asleep"].tolist())
            assert t["timers"] == d["timers"], (name, t["step"], "timers", t["timers"], d["timers"])
    if sc.claims:
        sc.claims(trace, sc)


# ------------------------------------------------------------------------------------------------ leg B: oracle against the real engine
needs_engine = pytest.mark.skipif(ob.ref() is None, reason="oracle/_ref/libedynref.so not built (needs the reference's source at build time)")


@needs_engine
@pytest.mark.parametrize("name", ENGINE)
def test_oracle_islands_match_the_engine(name):
    """The real engine and the oracle in lock-step (the oracle visits constraints in the engine's order, both call the C library's
    trigonometry): state, sleeping flags and the island partition after every step of the script."""
    sc = ig.by_name(name)
    ob.set_libm_trig(True)
    try:
        ref, orc, book = EngineSide(sc), OracleSide(sc, order=ob.ORDER_EXTERNAL), _Book(sc)
        for step in range(1, sc.steps + 1):
            for act in sc.script.get(step, []):
                ref.apply(act); orc.apply(act); book.apply(act)
            ref.w.step(1)
            orc.w.set_ext_order(*ref.w.get_solve_order())
            orc.w.set_ext_restitution_walk(*ref.w.get_restitution_walk())
            orc.w.step(1)
            assert not orc.w.ext_order_mismatch(), (name, step)
            p = book.proc()
            for f, a, b in zip(("pos", "orn", "linvel", "angvel"), ref.w.get_state(), orc.w.get_state()):
                assert np.array_equal(a[p].view(np.uint32), b[p].view(np.uint32)), (name, step, f)
            assert np.array_equal(ref.w.get_pairs(), orc.w.get_pairs()), (name, step, "pair keys")
            ra, oa = ref.w.get_asleep()[p], orc.w.get_asleep()[p]
            assert np.array_equal(ra, oa), (name, step, "sleeping flags", ra.tolist(), oa.tolist())
            assert np.array_equal(ref.w.get_derived()[2][p], orc.w.get_derived()[2][p]), (name, step, "island partition")
            assert ref.w.num_islands == orc.w.get_stats()["num_islands"], (name, step, "island count")
    finally:
        ob.set_libm_trig(False)


# ------------------------------------------------------------------------------------------------ leg C: device against oracle
def _device_run(name, monkeypatch=None, knobs=None, compare_state=True):
    """The scenario on the device beside the oracle's trace. Returns the relabel mode of every step: 'full', 'incremental' or None."""
    sc = scenario_with_info(name)
    trace, _, end_state = oracle_trace(name)
    if knobs:
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
    g, book = DeviceSide(sc), _Book(sc)
    if knobs:
        for k in knobs:
            monkeypatch.delenv(k)
    modes = []
    for t in trace:
        step = t["step"]
        for act in sc.script.get(step, []):
            g.apply(act); book.apply(act)
        before = g.w.debug_relabel_steps()
        g.step()
        after = g.w.debug_relabel_steps()
        assert sum(after) - sum(before) <= 1, (name, step, before, after)
        modes.append("full" if after[0] > before[0] else "incremental" if after[1] > before[1] else None)
        d = _observe(g, book, sc.sleeping)
        p = t["proc"]
        assert np.array_equal(d["pairs"], t["pairs"]), (name, step, "pair keys")
        want = ig.definition_labels(len(p), book.kind, book.removed, d["pairs"], _live_joints(sc, step))
        assert np.array_equal(d["labels"][p], want[p]), (name, step, "labels against the definition over the device's pairs", modes[-1])
        assert np.array_equal(d["labels"][p], t["labels"][p]), (name, step, "labels", modes[-1])
        assert d["num_islands"] == t["num_islands"], (name, step, "island count", d["num_islands"], t["num_islands"], modes[-1])
        if sc.sleeping:
            assert np.array_equal(d["asleep"][p], t["asleep"][p]), (name, step, "sleeping flags", d["asleep"].tolist(), t["asleep"].tolist())
            assert d["timers"] == t["timers"], (name, step, "timers", d["timers"], t["timers"], modes[-1])
            assert d["clock"] == t["clock"], (name, step, "clock")
    if compare_state:
        p = trace[-1]["proc"]
        for f, a, b in zip(("pos", "orn", "linvel", "angvel"), g.w.get_state(), end_state):
            assert np.array_equal(a[p].view(np.uint32), b[p].view(np.uint32)), (name, f)
    return sc, modes, g


RING = [f"ring4-rot{r}" for r in range(4)]
CHAINS = [n for n in NAMES if n.startswith("chain-")]
MANY_NEW = ["rain", "rain-sleeping", "funnel"]
PLAIN = [n for n in NAMES if n not in RING + CHAINS + MANY_NEW]   # every scenario runs on the device in exactly one of the four tests


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN)
def test_device_islands_match_the_oracle(name):
    """Every step of the scenario: labels, island count, sleeping flags, timers and clock equal the oracle's, the state at the end too.
    An edit - a joint added or removed, a body removed or appended - relabels in full in the step that follows it."""
    sc, modes, _ = _device_run(name)
    assert modes[0] == "full", (name, "the first step of a scene relabels in full")
    for step, acts in sc.script.items():
        if any(a[0] in ("add_joints", "remove_joints", "remove_bodies", "append") for a in acts):
            assert modes[step - 1] == "full", (name, step, modes[step - 1])
    if name.startswith("ring4-") and name.endswith("-split"):
        # the second loss splits the ring: whatever the first loss left as the certificate is a spanning tree, so the edge is in it
        assert modes[sc.info["split_step"] - 1] == "full", (name, sc.info["split_step"], modes[sc.info["split_step"] - 1])
    if name == "joints_only":
        # no manifold now or before, no edit, no sleeping: the island stage returns before it chooses a mode; the first contact is a new
        # edge on an intact (empty) certificate
        first = sc.info["first_contact"]
        assert modes[1:first - 1] == [None] * (first - 2), (name, modes)
        assert modes[first - 1] == "incremental", (name, first, modes)
    if name == "joints_only-leaves":
        # the only manifold is a certificate edge: its loss (pm != 0, M == 0) relabels in full; after it the early return again
        lost = sc.info["lost"]
        assert modes[lost - 1] == "full" and modes[lost:] == [None] * (len(modes) - lost), (name, lost, modes)
    if name == "sleeping_owner-filtered":
        # The sleeping owner's kept manifold - the only certificate edge - is seen by the owner's copy of its segment and by the awake
        # passer-by that reaches the owner: counted once, the certificate holds in every step and nothing is ever relabelled in full.
        assert "full" not in modes[1:], (name, [k for k, m in enumerate(modes, 1) if m == "full"])


@pytest.mark.gpu
def test_ring_takes_both_relabel_modes_when_it_loses_an_edge():
    """ring4 in its four rotations: labels, timers and sleeping flags as the oracle's at every step; and over the rotations the step
    that loses the edge is taken at least once incrementally (the edge was no certificate edge) and at least once in full (it was)."""
    at_loss = {}
    for r, name in enumerate(RING):
        sc, modes, _ = _device_run(name)
        at_loss[r] = modes[sc.info["loss_step"] - 1]
        assert all(m != "full" for k, m in enumerate(modes, 1) if k not in (1, sc.info["loss_step"])), (r, "a full relabel without a reason", modes)
    print(f"[island edges] ring4: relabel mode at the step that loses the edge, by rotation: {at_loss}")
    assert "incremental" in at_loss.values() and "full" in at_loss.values(), at_loss


COMPRESS_BIT = {"0": "RELABEL_COMPRESS0", "1": "RELABEL_COMPRESS1", "2": "RELABEL_COMPRESSN"}


@pytest.mark.gpu
@pytest.mark.parametrize("compress", ("0", "1", "2"))
@pytest.mark.parametrize("name", CHAINS)
def test_chain_relabels_in_full_under_every_compress_setting(monkeypatch, name, compress):
    """Chains of 300 and 1 025 null joints in three index orders under EDYNHIP_CC_COMPRESS = 0, 1, 2 (read when the context is created):
    the first step's forced relabel and, when the row beside the chain loses its certificate edge, a relabel the step chose itself. That
    one sets the path bit of the number of compress passes it ran: the setting's bit and neither of the other two."""
    sc, modes, g = _device_run(name, monkeypatch, {"EDYNHIP_CC_COMPRESS": compress})
    assert modes[0] == "full" and modes[sc.info["lost"] - 1] == "full", (name, sc.info["lost"], modes)
    assert g.w.debug_paths() & set(COMPRESS_BIT.values()) == {COMPRESS_BIT[compress]}, (name, compress, sorted(g.w.debug_paths()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", MANY_NEW)
def test_many_new_edges_in_one_step_are_hooked_incrementally(name):
    """rain: 9 216 pairs appear in one step - more than the 8 192 lanes of k_cc_hook_new and k_sleep_edges - and that step is
    incremental; 9 216 islands afterwards. In the sleeping world the lower layer sleeps until then and every island wakes in that step
    (claimed on the oracle's trace, held on the device by the comparison of every step). funnel: 512 islands hook under one root in one
    incremental step."""
    sc, modes, _ = _device_run(name)
    arrival = sc.info["arrival"]
    assert modes[arrival - 1] == "incremental", (name, arrival, modes)


@pytest.mark.gpu
def test_transplanted_world_continues_through_the_merge():
    """One step before the merge of merge3, the device world's state moves into a fresh world - set_state, set_manifolds, set_asleep,
    set_sleep_timers, the live joints - and both continue identically, and as the oracle, through the merge and into sleep."""
    name = "merge3-j2"
    sc = scenario_with_info(name)
    trace, _, _ = oracle_trace(name)
    cut = sc.info["merge_step"] - 1
    g, book = DeviceSide(sc), _Book(sc)
    for step in range(1, cut + 1):
        for act in sc.script.get(step, []):
            g.apply(act)
        g.step()
    twin_scene = dict(sc.scene)
    twin_scene["pos"], twin_scene["orn"], twin_scene["linvel"], twin_scene["angvel"] = g.w.get_state()
    twin_scene["joints"] = [ig.null_joint(a, b) for a, b in _live_joints(sc, cut)]
    tw = ig.Scenario("twin", twin_scene, sleeping=True, dt=sc.dt)
    t = DeviceSide(tw)
    t.w.set_state(*g.w.get_state())
    t.w.set_manifolds(g.w.get_manifolds())
    t.w.set_asleep(g.w.get_asleep())
    t.w.set_sleep_timers(*g.w.get_sleep_timers())
    for step in range(cut + 1, sc.steps + 1):
        g.step(); t.step()
        a, b, o = _observe(g, book, True), _observe(t, book, True), trace[step - 1]
        for x in (a, b):
            assert np.array_equal(x["labels"], o["labels"]) and x["num_islands"] == o["num_islands"], (step, "labels")
            assert np.array_equal(x["asleep"], o["asleep"]) and x["timers"] == o["timers"] and x["clock"] == o["clock"], (step, x["timers"], o["timers"])
        for x, y in zip(g.w.get_state(), t.w.get_state()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), step
    assert trace[-1]["asleep"][sc.info["X"] + sc.info["Y"] + [sc.info["Z"]]].all()
