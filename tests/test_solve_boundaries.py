"""The solve at the edges of its iteration counts and island sizes, against the CPU oracle, bit for bit.

tests/test_knob_paths.py holds every path that a knob or the manifold count selects to the oracle. The solve also branches on the
iteration counts and, on the island-fused kernels, on the size and shape of an island; this file puts a scene on each side of every
such boundary. Every comparison is with the oracle in coloured order and reference arithmetic: pairs, state (as uint32), applied joint
impulses (as uint32) where there are joints, and the manifolds at the end. There is no tolerance in this file. What makes a row sit on
its boundary (schedule, path bits, item counts, body spans, island counts) is asserted from get_stats(), debug_paths() and the scene
arrays, not assumed.

A. Iteration counts (compared at every step)
   kMaxDfPosIters = 8    up to 8 position iterations a contact-only world runs the dataflow position launches (one error array per
                         iteration); from 9 it falls to the per-colour position solve on the push schedule, and the mixed schedule is
                         ruled out: counts 8 and 9 (and 16) on the pile, on the pile beside rag dolls, and changed on a running world
   P == 0                no position launch at all; k_integrate / k_finish take the transforms from other places
   V == 0                the warm start only (dataflow launch with one sweep; island register path without the impulse store)
   early exit            an island below the position error threshold takes no part in later iterations (k_pos_flags, s_done of
                         k_island_position, the err_prev chain of the dataflow form): a pile that stops after its third iteration
                         beside a box sunk into the floor, which goes on
B. Island sizes on k_island_velocity / k_island_position (compared at steps 1, 2, 3 and every 10th)
   64 / 65 items         register path / sweep path, in one launch
   span 255 / 256        the bodies of a register-path island must lie within kIslBodySlots = 256 indices
   1024 / 1025 items     sorted list in LDS / in global scratch (kIslLdsItems)
   4096 / 4097 items     island-fused kernels / per-colour launches (kIslFusedLimit), also crossed by a running world
   > 4096 islands        a block takes several islands in sequence (kIslGrid) and reuses its LDS
   63 / 65 items with contact phases; contact_extras rows and a generic constraint, which force the sweep path at small size
   64 joint colours      the most there are (kMaxColours); 65 are an error, and the next world in the process is not affected

A world with shapes plans a step's schedule from the PREVIOUS step's island sizes, so its first step runs per colour whatever the
islands are: the island-fused schedule is asserted from step 2 on there. A world without shapes reads this step's sizes once and is
on its schedule from the first step."""
import functools
import math
import os

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from edyn_amd._capi import EdynHipError
from oracle import binding as ob
from test_knob_paths import _Env, _pile_and_ragdolls, _u32

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATAFLOW, ISLAND_FUSED, MIXED, PER_COLOUR = {1, 2, 6}, 3, 4, 5   # edynhip_stats::solve_schedule (EDYNHIP_SCHEDULE_*)
ERR_COLOURS = -5                                                   # EDYNHIP_ERR_COLOURS
NO_DATAFLOW, NO_FUSED = {"EDYNHIP_DATAFLOW": "0"}, {"EDYNHIP_ISLAND_FUSED": "0"}
PART_B_STEPS = (1, 2, 3, 10, 20, 30)


@pytest.fixture(autouse=True)
def _oracle_in_reference_arithmetic():
    ob.set_arithmetic(ob.ARITH_REFERENCE)
    yield
    ob.set_arithmetic(ob.ARITH_REFERENCE)


# ------------------------------------------------------------------ scene generators
def _chains(lengths, perm=None, x0=0.0, sign=1.0, jitter=0.02):
    """Joint-only chains as scenes.c5_chains lays them out (a static anchor, then amorphous links with inertia diag(0.01), joints
    alternating point / hinge), one chain per entry of `lengths`: an island has exactly as many items as its chain has links.
    perm: body index permutation (perm[old] = new), the joints' indices remapped with it. sign = -1 lays the chains out towards -x; jitter: largest yaw of a chain."""
    nb = sum(l + 1 for l in lengths)
    s = scenes._empty(nb)
    u = scenes.splitmix64_uniform(len(lengths), stream=11)
    inertia = np.diag([0.01, 0.01, 0.01]).astype(np.float32).reshape(9)
    far, near = (0.25 * sign, 0.0, 0.0), (-0.25 * sign, 0.0, 0.0)
    joints, base = [], 0
    for c, links in enumerate(lengths):
        yaw = (float(u[c]) * 2 - 1) * jitter
        az = 2.0 * c
        s["kind"][base] = scenes.KIND_STATIC
        s["pos"][base] = (x0, 10.0, az)
        k = np.arange(links)
        sl = slice(base + 1, base + 1 + links)
        s["pos"][sl] = np.stack([x0 + sign * 0.5 * (k + 0.5) * math.cos(yaw), np.full(links, 10.0), az + 0.5 * (k + 0.5) * math.sin(yaw)], 1)
        s["inertia"][sl] = inertia
        s["has_inertia"][sl] = 1
        for q in range(links):
            jt = scenes.JOINT_POINT if q % 2 == 0 else scenes.JOINT_HINGE
            joints.append((jt, base + q, base + 1 + q, (0.0, 0.0, 0.0) if q == 0 else far, near, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0)))
        base += links + 1
    s["joints"] = joints
    if perm is not None:
        perm = np.asarray(perm, np.int64)
        assert np.array_equal(np.sort(perm), np.arange(nb))
        out = {}
        for k, v in s.items():
            if k != "joints":
                out[k] = np.empty_like(v); out[k][perm] = v
        out["joints"] = [(j[0], int(perm[j[1]]), int(perm[j[2]])) + tuple(j[3:]) for j in joints]
        s = out
    return s


def _chain_sizes(sc):
    """Island sizes from the scene's own joint table: joints per connected component over the dynamic bodies."""
    parent = np.arange(len(sc["kind"]))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        return a
    dyn = sc["kind"] == scenes.KIND_DYNAMIC
    for j in sc["joints"]:
        if dyn[j[1]] and dyn[j[2]]:
            parent[find(j[1])] = find(j[2])
    roots = [find(j[1] if dyn[j[1]] else j[2]) for j in sc["joints"]]
    return sorted(np.unique(roots, return_counts=True)[1].tolist())


def _span_scene():
    """200 chains of two links. Four of them have their two dynamic bodies exactly 255 indices apart (the register path's body slots
    just hold them), four exactly 256 apart (they do not); the bodies of the other chains fill the gaps in their own order."""
    nb = 600
    perm = np.full(nb, -1, np.int64)
    for i in range(4):   # chain c: anchor 3 c, links 3 c + 1 and 3 c + 2
        perm[3 * i + 1], perm[3 * i + 2] = i, i + 255
        perm[3 * (4 + i) + 1], perm[3 * (4 + i) + 2] = 300 + i, 300 + i + 256
    free = np.setdiff1d(np.arange(nb), perm[perm >= 0])
    perm[perm < 0] = free
    return _chains([2] * 200, perm=perm)


def _island_spans(sc):
    """Per chain of two links: the distance between the indices of its two dynamic bodies (the joint between them names both)."""
    dyn = sc["kind"] == scenes.KIND_DYNAMIC
    return [abs(j[1] - j[2]) for j in sc["joints"] if dyn[j[1]] and dyn[j[2]]]


def _necklace(links):
    """`links` spheres of radius 0.1 resting on the plane along an arc, 0.3 apart (neighbours never touch), each linked to the next by a
    point joint at the midpoint: one island of links - 1 joints and `links` contacts."""
    s = scenes._empty(links + 1)
    scenes._add_plane(s)
    R = 6.0
    ang = np.arange(links) * (0.3 / R)
    p = np.stack([R * np.sin(ang), np.full(links, 0.1), R * (1 - np.cos(ang))], 1).astype(np.float32)
    s["pos"][1:] = p
    s["shape_type"][1:] = scenes.SHAPE_SPHERE
    s["shape_param"][1:] = (0.1, 0, 0, 0)
    rng = np.random.default_rng(5)
    s["linvel"][1:] = (rng.normal(size=(links, 3)) * (0.3, 0.0, 0.3)).astype(np.float32)
    s["angvel"][1:] = (rng.normal(size=(links, 3)) * 2.0).astype(np.float32)
    for i in range(links - 1):
        mid = (p[i].astype(np.float64) + p[i + 1]) / 2
        s["joints"].append((scenes.JOINT_POINT, 1 + i, 2 + i, tuple(mid - p[i]), tuple(mid - p[i + 1]), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0)))
    return s


def _hub(spokes):
    """One dynamic amorphous hub with `spokes` dynamic amorphous bodies around it, a point joint each: every joint shares the hub, so
    every joint needs a colour of its own."""
    s = scenes._empty(spokes + 1)
    ang = np.arange(spokes) * (2 * np.pi / spokes)
    s["pos"][0] = (0, 10, 0)
    s["pos"][1:] = np.stack([np.cos(ang), np.full(spokes, 10.0), np.sin(ang)], 1)
    s["inertia"][:] = np.diag([0.01, 0.01, 0.01]).astype(np.float32).reshape(9)
    s["inertia"][0] *= 50
    s["mass"][0] = 20.0
    s["has_inertia"][:] = 1
    rng = np.random.default_rng(8)
    s["linvel"][1:] = (rng.normal(size=(spokes, 3)) * 0.5).astype(np.float32)
    s["angvel"][:] = (rng.normal(size=(spokes + 1, 3)) * 1.5).astype(np.float32)
    for i in range(spokes):
        d = s["pos"][1 + i] - s["pos"][0]
        s["joints"].append((scenes.JOINT_POINT, 0, 1 + i, tuple(0.5 * d), tuple(-0.5 * d), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0)))
    return s


SETTLE_STEPS, SUNK_DEPTH = 240, 0.05


@functools.lru_cache(maxsize=None)
def _early_exit_scene(joint):
    """A 3x3x3 pile as the oracle leaves it after SETTLE_STEPS steps beside one box started SUNK_DEPTH inside the floor. After 120 steps the
    brick-offset pile is still falling apart (3.9 m/s, 1 cm of penetration: its islands do not stop early); after 240 it lies in a few
    islands that creep at 0.7 m/s at most; all of them are below the position error threshold by their THIRD iteration and not all by
    their second - a run of 3 and a run of 8 iterations agree on the pile, a run of 2 does not - while the sunk box keeps correcting to the last iteration. joint:
    a point joint between the two bricks that lie closest, at the midpoint between them - the world then has joints and runs on the
    island-fused schedule."""
    pile = scenes.box_pile(3, 3, 3)
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(pile)
    o.step(SETTLE_STEPS)
    for f, a in zip(("pos", "orn", "linvel", "angvel"), o.get_state()):
        pile[f] = a.copy()
    box = scenes.subset(pile, np.array([1]))
    box["pos"][0] = (8.0, 0.5 - SUNK_DEPTH, 0.0)
    box["orn"][0] = (0, 0, 0, 1)
    box["linvel"][0] = 0; box["angvel"][0] = 0
    sc = scenes.merge(pile, box)
    if joint:
        d = np.linalg.norm(sc["pos"][1:-1, None] - sc["pos"][None, 1:-1], axis=2) + 1e9 * np.eye(len(sc["kind"]) - 2)
        a, b = (int(x) + 1 for x in np.unravel_index(np.argmin(d), d.shape))
        mid = (sc["pos"][a].astype(np.float64) + sc["pos"][b]) / 2

        def local(i):   # the world point `mid` in body i's frame
            q = sc["orn"][i].astype(np.float64); u, w = -q[:3], q[3]
            v = mid - sc["pos"][i]
            t = 2 * np.cross(u, v)
            return tuple(v + w * t + np.cross(u, t))
        sc["joints"] = [(scenes.JOINT_POINT, a, b, local(a), local(b), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0))]
    # the scene holds both behaviours, shown on the oracle alone: one step at 3 and at 8 position iterations
    first = []
    for pos in (3, 8, 2):
        w = ob.World(vel_iters=10, pos_iters=pos, order=ob.ORDER_COLOURED)
        w.add_bodies(sc)
        w.step(1)
        first.append([x.copy() for x in w.get_state()])
    sunk = len(sc["kind"]) - 1
    for x, y in zip(first[0], first[1]):
        assert np.array_equal(_u32(x[:sunk]), _u32(y[:sunk])), "the settled pile did not stop after its first position iterations"
    assert not np.array_equal(_u32(first[0][0][sunk]), _u32(first[1][0][sunk])), "the sunk box did not go on correcting"
    assert not np.array_equal(_u32(first[0][0][:sunk]), _u32(first[2][0][:sunk])), "the pile did not need its third iteration"
    return sc


def _extras_both(n):
    """The materials of test_contact_extras_bit_exact, kind "both", by body index."""
    return {i: dict(spin=0.03, roll=0.04, stiffness=6000.0, damping=80.0) if i % 2 == 0 else (dict(roll=0.02) if i % 4 == 1 else {}) for i in range(n)}


def _setup_extras(w, sc, device):
    n = len(sc["kind"])
    ex = _extras_both(n)
    if device:
        cols = [np.array([ex[i].get(k, d) for i in range(n)], np.float32) for k, d in (("spin", 0.0), ("roll", 0.0), ("stiffness", 1e18), ("damping", 1e18))]
        w.set_material_extras(0, *cols)
    else:
        for i, kw in ex.items():
            if kw:
                w.set_material_extras(i, **kw)


GENERIC_JOINT = 15


def _necklace_generic():
    sc = _necklace(32)
    sc["joints"][GENERIC_JOINT] = (scenes.JOINT_GENERIC,) + tuple(sc["joints"][GENERIC_JOINT][1:])
    return sc


def _setup_generic(w, sc, device):
    """The degrees of freedom of test_generic_constraint_bit_exact (its joint 0), the frame's first axis along the link."""
    from test_reference_engine import _frame
    j = sc["joints"][GENERIC_JOINT]
    fr = _frame(sc["pos"][j[2]] - sc["pos"][j[1]])
    lin = [[1, -0.05, 0.08, 0.2, 0.02, 300.0, 0.01, 0.0, 50.0, 0.5], [1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.02, 0.0, 0.0, 0.3]]
    ang = [[1, -0.05, 0.06, 0.3, 0.02, 2.0, 0.01, 0.01, 0.5, 0.02], [1, -0.4, 0.4, 0.0, 0.0, 0.0, 0.0, 0.0, 0.3, 0.0], [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.005, 0.0, 0.2, 0.01]]
    w.set_generic_definition(GENERIC_JOINT, fr, fr, lin + ang)


def _ragdolls():
    return scenes.figures(scenes.load_figure(os.path.join(GOLDEN, "ragdoll_capsule.npz")), 2, 2, pitch=1.6)


LENGTHS_64 = [1, 2, 63, 64, 65, 66, 128]
LENGTHS_LDS = [1023, 1024, 1025, 3, 5, 17]
LENGTHS_MANY = [66 if c % 64 == 63 else 2 for c in range(4200)]

# name -> (make the scene, what the scene needs after upload: f(world, scene, is_device) or None)
SCENES = {
    "mixed5": (lambda: scenes.box_pile(5, 5, 5, mixed=True), None),
    "ragdolls": (_ragdolls, None),
    "chains8x8": (lambda: scenes.c5_chains(8, 8), None),
    "pile_and_ragdolls": (_pile_and_ragdolls, None),
    "early_exit": (lambda: _early_exit_scene(False), None),
    "early_exit_joint": (lambda: _early_exit_scene(True), None),
    "chains_64": (lambda: _chains(LENGTHS_64), None),
    "chains_span": (_span_scene, None),
    "chains_lds": (lambda: _chains(LENGTHS_LDS), None),
    "chain_4096": (lambda: _chains([4096]), None),
    "chain_4097": (lambda: _chains([4097]), None),
    "chains_many": (lambda: _chains(LENGTHS_MANY), None),
    "necklace32": (lambda: _necklace(32), None),
    "necklace33": (lambda: _necklace(33), None),
    "necklace32_extras": (lambda: _necklace(32), _setup_extras),
    "necklace32_generic": (_necklace_generic, _setup_generic),
    "hub64": (lambda: _hub(64), None),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name][0]()


def _settings(w, name, device):
    sc = _scene(name)
    scenes.apply_figure_settings(w, sc)   # (a scene without figures has none)
    if SCENES[name][1]:
        SCENES[name][1](w, sc, device)


# ------------------------------------------------------------------ oracle beside device
def _snapshot(w, joints, generic=False):
    return dict(pairs=w.get_pairs().copy(), state=[a.copy() for a in w.get_state()], impulses=w.get_joint_impulses().copy() if joints else None,
                impulses24=w.get_joint_impulses24().copy() if generic else None)


def _assert_same(got, want, what):
    assert np.array_equal(got["pairs"], want["pairs"]), (what, "pairs")
    for a, b, f in zip(got["state"], want["state"], ("pos", "orn", "linvel", "angvel")):
        assert np.array_equal(_u32(a), _u32(b)), (what, f)
    for f in ("impulses", "impulses24"):
        if want[f] is not None:
            assert np.array_equal(_u32(got[f]), _u32(want[f])), (what, "joint " + f)


def _assert_manifolds(w, manifolds, what):
    from test_gpu_parity import assert_manifolds_equal
    assert_manifolds_equal(w.get_manifolds(), manifolds, what=what)


@functools.lru_cache(maxsize=None)
def _oracle_run(name, vel, pos, steps, at):
    """The oracle's trajectory of a scene at the steps `at` (None: every step), shared (never changed) by the rows of the scene."""
    sc = _scene(name)
    o = ob.World(vel_iters=vel, pos_iters=pos, order=ob.ORDER_COLOURED)
    o.add_bodies(sc)
    _settings(o, name, False)
    traj = {}
    for s in range(1, steps + 1):
        o.step(1)
        if at is None or s in at:
            traj[s] = _snapshot(o, bool(sc.get("joints")), name.endswith("generic"))
    for s, t in traj.items():
        assert all(np.isfinite(a).all() for a in t["state"]), (name, s, "the oracle's state is not finite")
    return traj, o.get_manifolds().copy(), o.get_stats()


def _device_world(monkeypatch, name, vel, pos, knobs, **cfg):
    sc = _scene(name)
    with _Env(monkeypatch, knobs):
        w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=vel, num_solver_position_iterations=pos, **cfg))
        w.set_scene(sc)
        _settings(w, name, True)
    return w


def _run(monkeypatch, name, vel=10, pos=3, steps=30, knobs={}, at=None):
    """One device world of the scene under the knobs, stepped beside the oracle's trajectory. Returns the per-step state, stats and
    path sets for the row's structural assertions and for device-with-device comparisons."""
    sc = _scene(name)
    traj, manifolds, ostats = _oracle_run(name, vel, pos, steps, at)
    w = _device_world(monkeypatch, name, vel, pos, knobs)
    what = (name, vel, pos, tuple(sorted(knobs)))
    states, stats, paths = [], [], []
    for s in range(1, steps + 1):
        w.step_simulation(1)
        got = _snapshot(w, bool(sc.get("joints")), name.endswith("generic"))
        states.append(got["state"]); stats.append(w.get_stats()); paths.append(w.debug_paths())
        if s in traj:
            _assert_same(got, traj[s], what + (s,))
    _assert_manifolds(w, manifolds, what)
    return dict(states=states, stats=stats, paths=paths, schedule=[st["solve_schedule"] for st in stats], oracle_stats=ostats, world=w)


def _assert_devices_equal(a, b, what):
    for s, (x, y) in enumerate(zip(a["states"], b["states"]), 1):
        for p, q in zip(x, y):
            assert np.array_equal(_u32(p), _u32(q)), (what, s)


def _moves(r):
    return not np.array_equal(_u32(r["states"][0][0]), _u32(r["states"][-1][0]))


# ------------------------------------------------------------------ A. iteration counts on every schedule
COUNTS = [(0, 0), (0, 3), (1, 1), (10, 0), (10, 1), (10, 8), (10, 9), (10, 16)]
A_ROWS = ([("mixed5", {}, c, 30) for c in COUNTS] + [("mixed5", NO_DATAFLOW, c, 30) for c in ((0, 0), (10, 0), (10, 9))] +
          [("ragdolls", {}, c, 30) for c in COUNTS] + [("chains8x8", {}, c, 30) for c in ((0, 3), (10, 0), (10, 9))] +
          [("pile_and_ragdolls", {}, c, 20) for c in ((10, 8), (10, 9))])


def _a_id(row):
    return "%s%s-v%dp%d" % (row[0], "-" + ",".join(k.replace("EDYNHIP_", "") + "=" + v for k, v in row[1].items()) if row[1] else "", row[2][0], row[2][1])


def _check_counts_row(name, knobs, vel, pos, r):
    sched, paths = r["schedule"], r["paths"][-1]
    if name == "mixed5" and not knobs:
        assert all(s in DATAFLOW for s in sched), sched
        assert ("POS_COLOUR_PUSH" in paths) == (pos > 8), (pos, sorted(paths))   # the dataflow position launches end at kMaxDfPosIters
        if pos == 0:
            assert not ({"POS_COLOUR_PUSH", "POS_MULTI_ROUND"} & paths), sorted(paths)
        assert "PER_COLOUR" not in paths
        assert _moves(r)
    elif name == "mixed5":
        assert "PER_COLOUR" in paths and all(s == PER_COLOUR for s in sched), (sched, sorted(paths))
        assert not ({"VEL_LANES1", "VEL_LANES2", "VEL_LANES4"} & paths)
        assert _moves(r)
    elif name == "ragdolls":
        assert all(st["num_joints"] == 144 for st in r["stats"]) and r["stats"][-1]["num_active_manifolds"] > 0   # joints, and contacts once the figures reach the floor
        assert "ISLAND_FUSED" in paths and "MIXED" not in paths and all(s == ISLAND_FUSED for s in sched[1:]), (sched, sorted(paths))
    elif name == "chains8x8":
        assert all(st["num_active_manifolds"] == 0 and st["num_manifolds"] == 0 and st["num_joints"] == 64 for st in r["stats"])   # na == 0: the island lists are kept
        assert all(s == ISLAND_FUSED for s in sched) and "PER_COLOUR" not in paths, (sched, sorted(paths))
        assert _moves(r)
    elif name == "pile_and_ragdolls":
        if pos <= 8:
            assert "MIXED" in paths and sched[-1] == MIXED, (sched, sorted(paths))
        else:   # more position iterations than the dataflow position launches take: no mixed schedule
            assert "MIXED" not in paths and "PER_COLOUR" in paths and MIXED not in sched, (sched, sorted(paths))


@pytest.mark.parametrize("row", A_ROWS, ids=[_a_id(r) for r in A_ROWS])
def test_iteration_counts_bit_exact(monkeypatch, row):
    name, knobs, (vel, pos), steps = row
    r = _run(monkeypatch, name, vel, pos, steps, knobs)
    _check_counts_row(name, knobs, vel, pos, r)


# position iterations 3 -> 8 -> 9 -> 0 -> 3 and velocity iterations 10 -> 0 -> 1 -> 10, one change at a time, 10 steps after each
CHANGES = [{}, dict(position_iterations=8), dict(velocity_iterations=0), dict(position_iterations=9), dict(velocity_iterations=1),
           dict(position_iterations=0), dict(velocity_iterations=10), dict(position_iterations=3)]


@pytest.mark.parametrize("name", ["mixed5", "ragdolls"])
def test_iteration_counts_changed_on_a_running_world_bit_exact(monkeypatch, name):
    sc = _scene(name)
    vel, pos = 10, 3
    w = _device_world(monkeypatch, name, vel, pos, {})
    o = ob.World(vel_iters=vel, pos_iters=pos, order=ob.ORDER_COLOURED)
    o.add_bodies(sc)
    _settings(o, name, False)
    step = 0
    for change in CHANGES:
        if change:
            vel, pos = change.get("velocity_iterations", vel), change.get("position_iterations", pos)
            w.set_params(**change)
            o.set_params(1 / 60, vel, pos)
        for k in range(10):
            before = w.debug_paths()
            w.step_simulation(1); o.step(1)
            step += 1
            _assert_same(_snapshot(w, bool(sc.get("joints"))), _snapshot(o, bool(sc.get("joints"))), (name, step, vel, pos))
            sched = w.get_stats()["solve_schedule"]
            if name == "mixed5":
                assert sched in DATAFLOW, (step, sched)
                # the bit appears in the first step with more than kMaxDfPosIters position iterations, and in no step before it
                appeared = "POS_COLOUR_PUSH" in w.debug_paths() and "POS_COLOUR_PUSH" not in before
                assert appeared == (change == dict(position_iterations=9) and k == 0), (step, pos, sorted(w.debug_paths()))
            elif step > 1:
                assert sched == ISLAND_FUSED, (step, sched)
    _assert_manifolds(w, o.get_manifolds(), name)
    assert (vel, pos) == (10, 3) and step == 80


EARLY_ROWS = [(v, p) for v in ("dataflow", "per_colour", "fused") for p in (2, 3, 8, 9)]


@pytest.mark.parametrize("variant,pos", EARLY_ROWS, ids=["%s-p%d" % r for r in EARLY_ROWS])
def test_position_solve_early_exit_bit_exact(monkeypatch, variant, pos):
    """A settled island stops after the iteration that found it below the threshold, a sunk box beside it goes on: the generator
    asserts on the oracle that the scene holds both (_early_exit_scene), then the device is held to the oracle on each schedule."""
    name = "early_exit_joint" if variant == "fused" else "early_exit"
    r = _run(monkeypatch, name, 10, pos, 20, NO_DATAFLOW if variant == "per_colour" else {})
    sched, paths = r["schedule"], r["paths"][-1]
    assert r["stats"][0]["num_islands"] == r["oracle_stats"]["num_islands"]
    if variant == "dataflow":
        assert all(s in DATAFLOW for s in sched) and ("POS_COLOUR_PUSH" in paths) == (pos > 8), (sched, sorted(paths))
    elif variant == "per_colour":
        assert all(s == PER_COLOUR for s in sched) and "PER_COLOUR" in paths, (sched, sorted(paths))
    else:
        assert r["stats"][0]["num_joints"] == 1
        assert all(s == ISLAND_FUSED for s in sched[1:]) and "ISLAND_FUSED" in paths and "MIXED" not in paths, (sched, sorted(paths))


# ------------------------------------------------------------------ B. island sizes on the fused kernels
def _assert_joint_only(r, sc, fused=True):
    """A world of chains: no contact, every joint live, one island per chain, on the island-fused schedule from the first step."""
    for st in r["stats"]:
        assert st["num_joints"] == len(sc["joints"]) and st["num_active_manifolds"] == 0, st
    assert r["stats"][0]["num_islands"] == r["oracle_stats"]["num_islands"]
    if fused:
        assert all(s == ISLAND_FUSED for s in r["schedule"]) and "PER_COLOUR" not in r["paths"][-1], r["schedule"]
    else:
        assert all(s == PER_COLOUR for s in r["schedule"]) and "ISLAND_FUSED" not in r["paths"][-1], r["schedule"]


def test_islands_of_64_and_65_items_in_one_launch_bit_exact(monkeypatch):
    sc = _scene("chains_64")
    assert _chain_sizes(sc) == sorted(LENGTHS_64) and {63, 64, 65} <= set(LENGTHS_64)   # both sides of the register path's size limit
    fused = _run(monkeypatch, "chains_64", at=PART_B_STEPS)
    _assert_joint_only(fused, sc)
    assert fused["stats"][0]["num_islands"] >= len(LENGTHS_64)
    per_colour = _run(monkeypatch, "chains_64", knobs=NO_FUSED, at=PART_B_STEPS)
    _assert_joint_only(per_colour, sc, fused=False)
    _assert_devices_equal(fused, per_colour, "chains_64")


def test_island_body_span_of_255_and_256_bit_exact(monkeypatch):
    sc = _scene("chains_span")
    spans = _island_spans(sc)
    assert len(spans) == 200 and spans.count(255) == 4 and spans.count(256) == 4 and max(spans) == 256   # kIslBodySlots = 256: hi - lo < 256
    assert _chain_sizes(sc) == [2] * 200
    _assert_joint_only(_run(monkeypatch, "chains_span", at=PART_B_STEPS), sc)


def test_islands_of_1024_and_1025_items_bit_exact(monkeypatch):
    sc = _scene("chains_lds")
    assert _chain_sizes(sc) == sorted(LENGTHS_LDS) and {1023, 1024, 1025} <= set(LENGTHS_LDS)   # kIslLdsItems = 1024
    _assert_joint_only(_run(monkeypatch, "chains_lds", at=PART_B_STEPS), sc)


@pytest.mark.parametrize("links", [4096, 4097])
def test_island_at_the_fused_limit_bit_exact(monkeypatch, links):
    sc = _scene("chain_%d" % links)
    assert _chain_sizes(sc) == [links]
    _assert_joint_only(_run(monkeypatch, "chain_%d" % links, at=PART_B_STEPS), sc, fused=links <= 4096)   # kIslFusedLimit = 4096, from the first step on


def test_island_grows_past_the_fused_limit_on_a_running_world_bit_exact(monkeypatch):
    """A chain of 4 090 links runs on the island-fused kernels. A chain of 10 links, laid out towards the first one's free end, and a
    joint between the two free ends are added to the running world: an island of 4 101 items, which the step after the edit must
    already solve per colour."""
    first = _chains([4090], jitter=0.0)
    second = _chains([10], x0=0.5 * 4090 + 5.0, sign=-1.0, jitter=0.0)
    n1, j1 = len(first["kind"]), len(first["joints"])
    shifted = [(j[0], j[1] + n1, j[2] + n1) + tuple(j[3:]) for j in second["joints"]]
    link = (scenes.JOINT_POINT, n1 - 1, n1 + 10, (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0))
    assert np.allclose(first["pos"][n1 - 1] + (0.25, 0, 0), second["pos"][10] - (0.25, 0, 0), atol=1e-3)   # the free ends meet
    both = dict(kind=np.concatenate([first["kind"], second["kind"]]), joints=first["joints"] + shifted + [link])
    assert _chain_sizes(first) == [4090] and _chain_sizes(both) == [4101]
    with _Env(monkeypatch, {}):
        w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, max_bodies=n1 + 11, max_joints=j1 + 11))
        w.set_scene(first)
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(first)

    def lockstep(steps, schedule, what):
        for s in range(1, steps + 1):
            w.step_simulation(1); o.step(1)
            assert w.get_stats()["solve_schedule"] == schedule, (what, s, w.get_stats())
            if s <= 3 or s % 10 == 0:
                got, want = _snapshot(w, True), _snapshot(o, True)
                assert np.isfinite(want["state"][0]).all()
                _assert_same(got, want, (what, s))
    lockstep(5, ISLAND_FUSED, "4090 links")
    assert "PER_COLOUR" not in w.debug_paths()
    assert w.add_scene(second) == n1
    assert w.add_joints(shifted + [link]) == j1
    second_shifted = dict(second, joints=shifted + [link])
    o.add_bodies(second_shifted)
    lockstep(20, PER_COLOUR, "4101 links")
    assert w.get_stats()["num_joints"] == 4101


def test_more_islands_than_workgroups_bit_exact(monkeypatch):
    sc = _scene("chains_many")
    sizes = _chain_sizes(sc)
    assert len(sizes) == 4200 and sizes.count(2) == 4200 - 65 and sizes.count(66) == 65
    assert LENGTHS_MANY[63] == 66 and LENGTHS_MANY[62] == 2   # register-path and sweep-path islands follow each other in a block's sequence
    r = _run(monkeypatch, "chains_many", at=PART_B_STEPS)
    _assert_joint_only(r, sc)
    assert r["stats"][0]["num_islands"] > 4096, r["stats"][0]   # kIslGrid = 4096 workgroups


def _assert_necklace(r, sc, links, every_step=True):
    st = r["stats"][0]
    assert st["num_joints"] == links - 1 and st["num_joints"] + st["num_active_manifolds"] == 2 * links - 1, st   # items of the one island
    items = [x["num_joints"] + x["num_active_manifolds"] for x in r["stats"]]
    if every_step:
        assert items == [2 * links - 1] * len(items), "a sphere left the plane or touched its neighbour"
    assert all(x["num_islands"] == 1 for x in r["stats"]) and max(items) == 2 * links - 1, items
    assert "ISLAND_FUSED" in r["paths"][-1] and "MIXED" not in r["paths"][-1] and all(s == ISLAND_FUSED for s in r["schedule"][1:]), r["schedule"]


@pytest.mark.parametrize("links", [32, 33])
def test_island_of_63_and_65_items_with_contact_phases_bit_exact(monkeypatch, links):
    name = "necklace%d" % links
    _assert_necklace(_run(monkeypatch, name, at=PART_B_STEPS), _scene(name), links)


@pytest.mark.parametrize("what", ["extras", "generic"])
def test_small_island_forced_onto_the_sweep_path_bit_exact(monkeypatch, what):
    """63 items, small enough for the register path, but with contact_extras rows (rwx != nullptr) or a generic constraint in the island."""
    name = "necklace32_" + what
    sc = _scene(name)
    r = _run(monkeypatch, name, at=PART_B_STEPS)
    _assert_necklace(r, sc, 32, every_step=what != "generic")   # (the generic constraint's spring lifts a sphere off the plane now and then: 62 items)
    if what == "generic":
        assert [j[0] for j in sc["joints"]].count(scenes.JOINT_GENERIC) == 1
        assert np.abs(r["world"].get_joint_impulses24()[GENERIC_JOINT]).max() > 0
    else:
        o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
        o.add_bodies(sc)
        _settings(o, name, False)
        o.step(30)
        gx, ox = r["world"].get_point_extras(), o.get_point_extras()
        assert np.array_equal(_u32(gx), _u32(ox)) and (gx[..., :3] != 0).any()   # rolling / spinning impulses: the extras rows were solved


def test_64_joint_colours_bit_exact_and_65_refused(monkeypatch):
    sc = _scene("hub64")
    assert len(sc["joints"]) == 64 and all(j[1] == 0 for j in sc["joints"]) and (sc["kind"] == scenes.KIND_DYNAMIC).all()

    def run_64(knobs):
        r = _run(monkeypatch, "hub64", knobs=knobs, at=PART_B_STEPS)
        assert all(st["num_joint_colours"] == 64 and st["num_joints"] == 64 for st in r["stats"])   # 64 joint phases, one island of 64 items
        assert r["oracle_stats"]["num_joint_colours"] == 64
        return r
    fused = run_64({})
    assert all(s == ISLAND_FUSED for s in fused["schedule"]), fused["schedule"]
    per_colour = run_64(NO_FUSED)
    assert all(s == PER_COLOUR for s in per_colour["schedule"]), per_colour["schedule"]
    _assert_devices_equal(fused, per_colour, "hub64")
    # one spoke more: the joints cannot be coloured
    with _Env(monkeypatch, {}):
        bad = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3))
        with pytest.raises(EdynHipError) as err:
            bad.set_scene(_hub(65))
            bad.step_simulation(1)
    assert err.value.code == ERR_COLOURS and "joint colours" in str(err.value), str(err.value)
    assert "joint colours" in bad._L.edynhip_last_error(bad._h).decode()
    bad.detach()
    again = run_64({})   # a fresh world in the same process is not affected
    _assert_devices_equal(fused, again, "hub64 after the refused world")
