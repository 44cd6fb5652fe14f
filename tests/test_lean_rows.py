"""Lean contact rows (solver.hip SolvePlan::lean): a contact-only world whose velocity solve is one dataflow launch
stores three planes per row instead of five, and the dataflow kernels rebuild I^-1 J_ang before their wait from a lane-indexed copy of the
two inverse inertias. The rebuilt product is the stored product's mul(), so nothing a step computes may change by a single bit:
  * lean rows on, every dataflow kernel (EDYNHIP_DF_LANES 1, 2, 4), against the oracle's coloured order after 1 and after 20 steps: state
    and manifolds (normal and both friction impulses among their fields);
  * lean rows off (init_config(full_contact_rows=True), edynhip.h EDYNHIP_FLAG_FULL_CONTACT_ROWS) gives the same bytes;
  * the schedules that keep full rows - per colour (EDYNHIP_DATAFLOW=0), mixed (a hinge beside a pile), contact_extras - report full rows and
    give the same bytes with the switch either way; so does the fused arithmetic on lean rows.
Scenes: box_pile(6, 6, 6) has four-, three- and two-point manifolds, wave-tasks that straddle a point-count boundary (the predicated forms)
and a static plane (one side without inverse mass); its mixed form adds one-point sphere manifolds (the NP = 1 form); 40 boxes are less than
one wave-task. Everything is bit-exact: there is no tolerance in this file."""
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from oracle import binding as ob

pytestmark = pytest.mark.gpu
STEPS = (1, 20)
DATAFLOW, MIXED, PER_COLOUR = {1, 2, 6}, 4, 5   # edynhip_stats::solve_schedule
LANES_SCHEDULE = {1: 2, 2: 1, 4: 6}
KNOBS = ("EDYNHIP_DF_LANES", "EDYNHIP_DATAFLOW")


def _hinge_beside_pile():
    """An 8x8x8 pile (more than 1 024 manifolds in islands without joints: the mixed schedule) and, 25 m away, two boxes on the plane joined
    by one hinge."""
    pair = scenes._empty(2)
    pair["pos"][:] = ((25.0, 0.505, 0.0), (26.2, 0.505, 0.0))
    pair["shape_type"][:] = scenes.SHAPE_BOX
    pair["shape_param"][:, :3] = 0.5
    pair["joints"] = [(scenes.JOINT_HINGE, 0, 1, (0.6, 0.0, 0.0), (-0.6, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0))]
    return scenes.merge(scenes.box_pile(8, 8, 8), pair)


SCENES = {
    "pile6": (lambda: scenes.box_pile(6, 6, 6), 10),
    "mixed6": (lambda: scenes.box_pile(6, 6, 6, mixed=True), 20),
    "pile40": (lambda: scenes.box_pile(5, 4, 2), 10),
    "hinge_beside_pile": (_hinge_beside_pile, 10),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name][0]()


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's coloured order at STEPS: computed once per scene, shared and never changed."""
    o = ob.World(vel_iters=SCENES[name][1], pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(_scene(name))
    out, done = {}, 0
    for s in STEPS:
        o.step(s - done); done = s
        out[s] = ([a.copy() for a in o.get_state()], o.get_manifolds().copy())
    return out


_runs = {}


def _device(monkeypatch, name, full, knobs=(), extras=False, **cfg):
    """State, manifolds, schedule and lean_rows of a device world at STEPS (one run per setting, shared by the tests)."""
    key = (name, full, tuple(knobs), extras, tuple(sorted(cfg.items())))
    if key in _runs:
        return _runs[key]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs:
        monkeypatch.setenv(k, v)
    sc = _scene(name)
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=SCENES[name][1], num_solver_position_iterations=3, full_contact_rows=full, **cfg))
    w.set_scene(sc)
    for k, _ in knobs:   # (the library reads them when the context is created)
        monkeypatch.delenv(k, raising=False)
    if extras:   # rolling and spinning friction on every body, a soft contact on every fourth: contact_extras rows
        n = len(sc["kind"])
        soft = (np.arange(n) % 4) == 1
        w.set_material_extras(0, spin=np.full(n, 0.02, np.float32), roll=np.full(n, 0.01, np.float32),
                              stiffness=np.where(soft, 2.0e4, 1e18).astype(np.float32), damping=np.where(soft, 2.0e2, 1e18).astype(np.float32))
    out, done = {}, 0
    for s in STEPS:
        w.step_simulation(s - done); done = s
        st = w.get_stats()
        out[s] = dict(state=[a.copy() for a in w.get_state()], manifolds=w.get_manifolds().copy(), schedule=st["solve_schedule"], lean=st["lean_rows"])
    _runs[key] = out
    return out


def _assert_bytes_equal(a, b, what):
    for s in STEPS:
        for x, y, f in zip(a[s]["state"], b[s]["state"], ("pos", "orn", "linvel", "angvel")):
            assert np.array_equal(_u32(x), _u32(y)), (what, s, f)
        assert a[s]["manifolds"].tobytes() == b[s]["manifolds"].tobytes(), (what, s, "manifolds")


@pytest.mark.parametrize("lanes", (1, 2, 4))
@pytest.mark.parametrize("name", ("pile6", "mixed6", "pile40"))
def test_lean_rows_against_the_oracle_and_against_full_rows(monkeypatch, name, lanes):
    from test_gpu_parity import assert_manifolds_equal
    knobs = (("EDYNHIP_DF_LANES", str(lanes)),)
    lean, full, want = _device(monkeypatch, name, False, knobs), _device(monkeypatch, name, True, knobs), _oracle(name)
    for s in STEPS:
        assert lean[s]["schedule"] == full[s]["schedule"] == LANES_SCHEDULE[lanes], (lean[s]["schedule"], full[s]["schedule"])   # the kernel asked for ran
        assert lean[s]["lean"] == 1 and full[s]["lean"] == 0   # and the switch selected what it says
        for a, b, f in zip(lean[s]["state"], want[s][0], ("pos", "orn", "linvel", "angvel")):
            assert np.array_equal(_u32(a), _u32(b)), (name, lanes, s, f)
        assert_manifolds_equal(lean[s]["manifolds"], want[s][1], what=(name, lanes, s))   # impulses: normal_impulse, friction_impulse[2]
        assert (lean[s]["manifolds"]["pt"]["normal_impulse"] != 0).any()
    _assert_bytes_equal(lean, full, (name, lanes))


def test_the_scenes_reach_every_form_of_the_kernels():
    """What the scenes are chosen for: every point count, classes that end inside a wave-task, a side without inverse mass."""
    for name, counts in (("pile6", {2, 3, 4}), ("mixed6", {1, 2, 3, 4})):
        m = _oracle(name)[20][1]
        act = m[m["num_points"] > 0]
        assert counts <= set(np.unique(act["num_points"])), (name, np.unique(act["num_points"]))
        sizes = np.unique(act["colour"].astype(np.int64) * 8 + act["num_points"], return_counts=True)[1]
        assert (sizes % 32 != 0).any() and len(act) > 64   # point-count classes that end inside a 32-manifold task, several tasks
        assert (act["body"] == 0).any()                    # the static plane
    m = _oracle("pile40")[20][1]
    assert 0 < (m["num_points"] > 0).sum() and len(_scene("pile40")["kind"]) == 41


def test_fused_arithmetic_on_lean_rows_equals_full_rows(monkeypatch):
    lean, full = _device(monkeypatch, "pile6", False, fused_velocity_rows=True), _device(monkeypatch, "pile6", True, fused_velocity_rows=True)
    assert all(lean[s]["lean"] == 1 and full[s]["lean"] == 0 and lean[s]["schedule"] in DATAFLOW for s in STEPS)
    _assert_bytes_equal(lean, full, "fused")
    plain = _device(monkeypatch, "pile6", False)
    assert not np.array_equal(_u32(plain[20]["state"][2]), _u32(lean[20]["state"][2]))   # (the other arithmetic did run)


@pytest.mark.parametrize("what", ("per_colour", "mixed", "extras"))
def test_schedules_that_keep_full_rows_do_not_change(monkeypatch, what):
    name = "hinge_beside_pile" if what == "mixed" else "pile6"
    kw = dict(knobs=(("EDYNHIP_DATAFLOW", "0"),)) if what == "per_colour" else dict(extras=True) if what == "extras" else {}
    dflt, full = _device(monkeypatch, name, False, **kw), _device(monkeypatch, name, True, **kw)
    for s in STEPS:
        assert dflt[s]["lean"] == 0 and full[s]["lean"] == 0, (what, s)   # full rows whatever the switch says
        assert dflt[s]["schedule"] == full[s]["schedule"]
    if what == "per_colour":
        assert all(dflt[s]["schedule"] == PER_COLOUR for s in STEPS)
    elif what == "mixed":
        assert dflt[20]["schedule"] == MIXED, dflt[20]["schedule"]
    else:
        assert all(dflt[s]["schedule"] not in DATAFLOW for s in STEPS)
        assert not np.array_equal(_u32(dflt[20]["state"][3]), _u32(_device(monkeypatch, "pile6", False)[20]["state"][3]))   # (the extras rows did act)
    _assert_bytes_equal(dflt, full, what)
