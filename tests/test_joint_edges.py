"""The joint rows at limit, wrap and degenerate poses (tests/jointposes.py), bit for bit.

CPU leg (not marked gpu; skipped where oracle/_ref was never built): every case, the oracle in ORDER_EXTERNAL against the real engine
in lock step - state, the 10 or 24 applied impulses and the tracked angle as uint32 at every step, the engine's state finite at every
step - and then the case's evidence that the edge was reached, on the engine's output.

GPU leg (marked gpu): the device against the oracle in coloured order and reference arithmetic, at every step: pairs, state,
get_joint_impulses / get_joint_impulses24 as uint32 (tracked angle included); the evidence again, on the oracle's output. There is no
tolerance in this file. Every case runs on the three forms of the joint solve, and which form ran is asserted from the schedule, the
path bits and the island's items:
  register   k_island_velocity's register path (jlane_*): island-fused schedule, an island of at most 64 items without a generic constraint
  sweep      k_island_velocity's sweep path (joint_solve_lane): the case's link also hangs on a generic constraint without any row (every
             degree of freedom free) that ties a further body to it - a generic constraint in the island rules the register path out
             (tests/test_solve_boundaries.py forces the sweep path the same way). The cases that hold a generic constraint are on this form already.
  per_colour EDYNHIP_ISLAND_FUSED=0: k_joint_solve and k_pos_joints
Then each case with one velocity iteration and no position iteration (the applied impulse is clamp(rhs * eff) of the prepared row: a
wrong row cannot be absorbed by later sweeps) and with one velocity and three position iterations (pos_joints_lane's gates, through the
state); all cases merged into worlds of 1, 127, 128 and 129 joints (k_prep_joints and k_prep_generic launch 128 lanes a block);
k_joint_reset_angle on a running world next to +-pi and beyond a turn; set_joint_warm_start with tracked angles of several turns."""
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from oracle import binding as ob
import jointposes as jp
from test_reference_engine import _joint_lockstep, pytestmark as needs_ref   # (the skipif of that file, used on the CPU leg only)

CASES = jp.cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _collect(world, generic):
    return dict(imp=world.get_joint_impulses().copy(), imp24=world.get_joint_impulses24().copy() if generic else None,
                state=[a.copy() for a in world.get_state()])


def _stack(steps, generic):
    return dict(imp=np.stack([s["imp"] for s in steps]), imp24=np.stack([s["imp24"] for s in steps]) if generic else None,
                state=[s["state"] for s in steps])


# ------------------------------------------------------------------ CPU leg: oracle against the real engine
@pytest.fixture
def libm_trig():   # test_reference_engine's fixture is autouse; the GPU leg of this file must stay on the correctly rounded trig
    ob.set_libm_trig(True)
    yield
    ob.set_libm_trig(False)


def _engine_lockstep(case):
    """test_reference_engine._joint_lockstep (state, impulses and tracked angle as uint32, the engine's state finite, at every step) on
    the case; returns the engine's per-step record, which the evidence reads."""
    sc, steps = case["scene"], []
    _joint_lockstep(sc, case["steps"], lambda w: jp.apply(w, sc), each_step=lambda s, ref, orc: steps.append(_collect(ref, case["generic"])))
    return _stack(steps, case["generic"])


@needs_ref
@pytest.mark.parametrize("name", NAMES)
def test_joint_edge_matches_the_real_engine(libm_trig, name):
    case = BY_NAME[name]
    out = _engine_lockstep(case)
    case["evidence"](case["scene"], out)


# ------------------------------------------------------------------ GPU leg: device against the oracle
from test_solve_boundaries import ISLAND_FUSED, NO_FUSED, PER_COLOUR, _chain_sizes   # noqa: E402
from test_knob_paths import _Env   # noqa: E402

FORMS = ("register", "sweep", "per_colour")
ALL_FREE = [[0] * 10] * 6


@pytest.fixture
def reference_arithmetic():
    ob.set_arithmetic(ob.ARITH_REFERENCE)
    yield
    ob.set_arithmetic(ob.ARITH_REFERENCE)


def _with_rider(sc):
    """The scene with one more dynamic body tied to joint 0's dynamic link by a generic constraint without rows: same island, no register path."""
    t = sc["joints"][0]
    link = t[2] if sc["kind"][t[2]] == scenes.KIND_DYNAMIC else t[1]
    rider = jp.bodies([scenes.KIND_DYNAMIC], [sc["pos"][link] + np.float32((0.0, 0.0, 0.75))])
    # scenes.merge adds len(sc["kind"]) to both body indices of the second scene's joints: link - n lands on `link`, 0 on the rider
    rider["joints"].append((scenes.JOINT_GENERIC, int(link) - len(sc["kind"]), 0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), jp.X, jp.X))
    rider["generic_defs"].append((0, jp.EYE, jp.EYE, ALL_FREE))
    return jp.merge(sc, rider)


@functools.lru_cache(maxsize=None)
def _form_scene(name, form):
    case = BY_NAME[name]
    return _with_rider(case["scene"]) if form == "sweep" and not case["generic"] else case["scene"]


def _has_generic(sc):
    return any(t[0] == scenes.JOINT_GENERIC for t in sc["joints"])


@functools.lru_cache(maxsize=None)
def _oracle_traj(name, form, vel, pos):
    """The oracle's trajectory of a case's scene, shared (never changed) by the rows that need it."""
    case, sc = BY_NAME[name], _form_scene(name, form)
    o = ob.World(vel_iters=vel, pos_iters=pos, order=ob.ORDER_COLOURED)
    o.add_bodies(sc); jp.apply(o, sc)
    steps = []
    for s in range(case["steps"]):
        o.step(1)
        steps.append(dict(_collect(o, True), pairs=o.get_pairs().copy()))
        assert all(np.isfinite(a).all() for a in steps[-1]["state"]), (name, s + 1)
    return steps


def _device(monkeypatch, sc, vel, pos, knobs):
    with _Env(monkeypatch, knobs):
        w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=vel, num_solver_position_iterations=pos))
        w.set_scene(sc); jp.apply(w, sc)
    return w


def _assert_step(w, want, what):
    assert np.array_equal(w.get_pairs(), want["pairs"]), (what, "pairs")
    for f, a, b in zip(("pos", "orn", "linvel", "angvel"), w.get_state(), want["state"]):
        assert np.array_equal(_u32(a), _u32(b)), (what, f, a, b)
    got = w.get_joint_impulses()
    assert np.array_equal(_u32(got), _u32(want["imp"])), (what, "impulses and tracked angle", got, want["imp"])
    assert np.array_equal(_u32(w.get_joint_impulses24()), _u32(want["imp24"])), (what, "24 impulse slots")


def _assert_form(w, sc, form):
    """The device reports the schedule and the path bits; between the register and the sweep path of k_island_velocity it reports nothing,
    so that choice is asserted from the kernel's own predicate restated on the scene (at most 64 items, body span below 256, no generic
    constraint in the island, no contact_extras rows), as tests/test_solve_boundaries.py does. The two paths are the same arithmetic: a
    device that took the other one against this predicate would not be noticed here."""
    st, paths = w.get_stats(), w.debug_paths()
    assert st["num_joints"] == len(sc["joints"]) and st["num_active_manifolds"] == 0, st
    if form == "per_colour":
        assert st["solve_schedule"] == PER_COLOUR and "PER_COLOUR" in paths and "ISLAND_FUSED" not in paths, (st, sorted(paths))
        return
    assert st["solve_schedule"] == ISLAND_FUSED and "ISLAND_FUSED" in paths and "PER_COLOUR" not in paths, (st, sorted(paths))
    assert max(_chain_sizes(sc)) <= 64 and len(sc["kind"]) < 256   # small enough for the register path, so only a generic constraint keeps an island off it
    assert _has_generic(sc) == (form == "sweep")


def _run_case(monkeypatch, name, form, vel=10, pos=3, evidence=True):
    case, sc = BY_NAME[name], _form_scene(name, form)
    want = _oracle_traj(name, form, vel, pos)
    w = _device(monkeypatch, sc, vel, pos, NO_FUSED if form == "per_colour" else {})
    for s in range(case["steps"]):
        w.step_simulation(1)
        _assert_step(w, want[s], (name, form, vel, pos, s + 1))
        _assert_form(w, sc, form)
    if evidence:
        case["evidence"](sc, _stack(want, True))


FORM_ROWS = [(n, f) for n in NAMES for f in FORMS if not (f == "register" and BY_NAME[n]["generic"])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form", FORM_ROWS, ids=["%s-%s" % r for r in FORM_ROWS])
def test_joint_edge_bit_exact_on_each_solve_form(monkeypatch, reference_arithmetic, name, form):
    _run_case(monkeypatch, name, form)


ONE_SWEEP_ROWS = [(n, f, p) for n, f in FORM_ROWS for p in (0, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,pos", ONE_SWEEP_ROWS, ids=["%s-%s-p%d" % r for r in ONE_SWEEP_ROWS])
def test_joint_edge_bit_exact_with_one_velocity_iteration(monkeypatch, reference_arithmetic, name, form, pos):
    """One sweep after the warm start: the applied impulse of the first step is clamp(rhs * eff) of the prepared row. pos = 3 compares the
    position solve's gates through the state. (The evidence belongs to the pose and the 10 / 3 iterations it was worked out for.)"""
    _run_case(monkeypatch, name, form, vel=1, pos=pos, evidence=False)
    if name == "hinge_mass_ratio_1e6" and pos == 3:
        # Ten sweeps leave a bump stop with an impulse of 0 (the row cannot pull, and a link that leaves is faster than the row's target
        # speed), one sweep does not: here the row goes away holding an impulse and comes back with it (limits +-0.4, bump stop 0.1).
        imp = np.stack([w["imp"][1] for w in _oracle_traj(name, form, 1, pos)])
        stale = np.flatnonzero((np.abs(imp[:, 9]) <= 0.3) & (imp[:, 6] != 0))
        assert len(stale) and (np.abs(imp[stale[0]:, 9]) > 0.3).any(), "no bump stop row came back with a stale impulse"


# ------------------------------------------------------------------ all cases in one world
MERGED_STEPS = 30


@functools.lru_cache(maxsize=None)
def _merged(total):
    """Cases repeated until the world has exactly `total` joints, in table order, so the types interleave in joint index order; each copy
    50 m further along z."""
    sc, k = None, 0
    while (len(sc["joints"]) if sc else 0) < total:
        c = CASES[k % len(CASES)]["scene"]
        k += 1
        if (len(sc["joints"]) if sc else 0) + len(c["joints"]) > total:
            continue   # a two-joint case that would overshoot: the next one-joint case fills the slot
        c = dict(c, pos=c["pos"] + np.float32((0.0, 0.0, 50.0 * k)))
        sc = jp.merge(sc, c) if sc else c
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("total", [1, 127, 128, 129])
@pytest.mark.parametrize("form", ["fused", "per_colour"])
def test_all_joint_edges_in_one_world_bit_exact(monkeypatch, reference_arithmetic, total, form):
    sc = _merged(total)
    types = [t[0] for t in sc["joints"]]
    assert len(types) == total
    if total > 100:
        assert len(set(types)) == 8 and sum(a != b for a, b in zip(types, types[1:])) > 20   # every type, interleaved
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(sc); jp.apply(o, sc)
    w = _device(monkeypatch, sc, 10, 3, NO_FUSED if form == "per_colour" else {})
    acted = np.zeros(total, bool)
    for s in range(MERGED_STEPS):
        o.step(1); w.step_simulation(1)
        want = dict(_collect(o, True), pairs=o.get_pairs())
        assert all(np.isfinite(a).all() for a in want["state"]), s + 1
        _assert_step(w, want, (total, form, s + 1))
        assert w.get_stats()["solve_schedule"] == (PER_COLOUR if form == "per_colour" else ISLAND_FUSED)
        acted |= np.abs(want["imp24"]).max(axis=1) > 0
    assert acted.sum() >= 0.9 * total, acted.sum()   # (a few cases are about a row that carries nothing)


# ------------------------------------------------------------------ k_joint_reset_angle, set_joint_warm_start
def _turning_pair():
    """A hinge (joint 0) and a cvjoint (joint 1), each between a kinematic anchor with a spin of 4 rad/s about the joint's axis and a link that a torque / friction row
    brings to that spin: the relative angle runs at 0.067 a step."""
    h = jp.hinge(jp.pair(scenes.KIND_KINEMATIC), pivA=(0.0, 0.0, 0.0), pivB=(0.0, 0.0, 0.0), params=[-100, 100, 0, 0, 0, 10.0, 0, 0.3, 0.5, 0.0])
    h["pos"][1] = h["pos"][0]
    h["angvel"][0] = (0, 0, 4.0)
    c = jp.pair(scenes.KIND_KINEMATIC)
    c["pos"][:, 2] += 5.0
    c["pos"][1] = c["pos"][0]
    c["joints"].append((scenes.JOINT_CVJOINT, 0, 1, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), jp.X, jp.X))
    c["joint_defs"].append((0, jp.EYE, jp.EYE, [-100, 100, 0, 0, 0, 10.0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]))
    c["angvel"][0] = (-4.0, 0, 0)
    return jp.merge(h, c)


RESET_HINGE = [-90, 110, 0, 0, 0, 10.0, 0, 0.3, 0.5, 0.0]
RESET_CV = [-90, 110, 0, 0, 0, 10.0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "per_colour"])
def test_reset_angle_next_to_pi_and_beyond_a_turn_bit_exact(monkeypatch, reference_arithmetic, form):
    """set_joint_params on a hinge and set_joint_definition on a cvjoint of a running world, at the first step at which the tracked angle
    is beyond a turn and the relative angle is within 0.05 of +-pi (the moment is read from the oracle): both sides recompute the angle
    from the poses (hinge_constraint.cpp:19-24, cvjoint_constraint.cpp:12-23) and are compared on."""
    sc = _turning_pair()
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(sc); jp.apply(o, sc)
    w = _device(monkeypatch, sc, 10, 3, NO_FUSED if form == "per_colour" else {})
    done = [False, False]
    for s in range(200):
        o.step(1); w.step_simulation(1)
        want = dict(_collect(o, True), pairs=o.get_pairs())
        _assert_step(w, want, (form, s + 1))
        _assert_form(w, sc, "per_colour" if form == "per_colour" else "register")
        for j in (0, 1):
            a = float(want["imp"][j, 9])
            wrapped = (a + np.pi) % (2 * np.pi) - np.pi
            if not done[j] and abs(a) > 2 * np.pi and np.pi - abs(wrapped) < 0.05:
                for x in (o, w):
                    x.set_joint_params(0, RESET_HINGE) if j == 0 else x.set_joint_definition(1, jp.EYE, jp.EYE, RESET_CV)
                got, exp = w.get_joint_impulses()[j, 9], o.get_joint_impulses()[j, 9]
                assert _u32(got) == _u32(exp) and np.pi - abs(float(exp)) < 0.05, (j, got, exp)   # back within (-pi, pi], next to the seam
                done[j] = True
    assert done == [True, True]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fused", "per_colour"])
def test_warm_start_with_tracked_angles_of_several_turns_bit_exact(monkeypatch, reference_arithmetic, form):
    """Tracked angles 7.0 and -9.5 (and impulses) carried into a fresh context: track_angle must go on from them, not from their
    normalised values. The hinge's limits [6.5, 8] put 2 pi below angle_min, the cvjoint's [-14, -12.4] hold -4 pi on the max side and in
    its bump stop: rows that a normalised angle would not produce."""
    sc = _turning_pair()
    sc["hinge_params"][0] = (0, [6.5, 8.0, 0, 0.2, 3.0, 0, 0, 0.3, 0.5, 0.0])
    sc["joint_defs"][0] = (1, jp.EYE, jp.EYE, [-14.0, -12.4, 0, 0.2, 3.0, 0.001, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    sc["angvel"][0] = (0, 0, 0.5); sc["angvel"][2] = (-0.5, 0, 0)
    imp = np.zeros((2, 24), np.float32)
    imp[0, 5], imp[1, 3] = 0.01, -0.02
    angles = np.array([7.0, -9.5], np.float32)
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(sc); jp.apply(o, sc)
    w = _device(monkeypatch, sc, 10, 3, NO_FUSED if form == "per_colour" else {})
    o.set_joint_warm_start(imp, angles); w.set_joint_warm_start(imp, angles)
    first = None
    for s in range(40):
        o.step(1); w.step_simulation(1)
        want = dict(_collect(o, True), pairs=o.get_pairs())
        _assert_step(w, want, (form, s + 1))
        _assert_form(w, sc, "per_colour" if form == "per_colour" else "register")
        first = want["imp"][:, 9].copy() if first is None else first
    # the relative angles start at 0: the tracked ones land on the multiple of 2 pi nearest to what was carried in
    assert abs(first[0] - 2 * np.pi) < 0.5 and abs(first[1] + 4 * np.pi) < 0.5, first   # (7.0 and -9.5 are 0.72 and 3.07 away)
