"""The one-pass narrowphase (k_np_contacts: detect + merge with the raw result handed over in LDS) against the two-kernel path
through the staging arrays (EDYNHIP_NP_FUSED=0, read when a world is created): the same scene stepped in one world of each kind,
manifolds and state bit for bit after every step.
"""
import os

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEPS = 60


def _world(scene, fused, **kw):
    """A world on the default (fused) path, or on the staged path: the knob is read once, at context creation."""
    before = os.environ.pop("EDYNHIP_NP_FUSED", None)
    try:
        if not fused:
            os.environ["EDYNHIP_NP_FUSED"] = "0"
        w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, **kw))
    finally:
        os.environ.pop("EDYNHIP_NP_FUSED", None)
        if before is not None:
            os.environ["EDYNHIP_NP_FUSED"] = before
    w.set_scene(scene)
    scenes.apply_figure_settings(w, scene)   # hinge limits, joint frames, exclusions: nothing to do for a scene without figures
    return w


def _assert_same(a, b, what):
    ma, mb = a.get_manifolds(), b.get_manifolds()
    assert len(ma) == len(mb), what
    assert np.array_equal(ma.view(np.uint8), mb.view(np.uint8)), what
    for name, x, y in zip(("pos", "orn", "linvel", "angvel"), a.get_state(), b.get_state()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, name)
    return ma


def _sorted_events(ev):
    return np.sort(ev, order=["step", "type", "body", "point_id"])


def _lockstep(scene, steps=STEPS, **kw):
    a, b = _world(scene, True, **kw), _world(scene, False, **kw)
    points = 0
    for s in range(1, steps + 1):
        a.step_simulation(1); b.step_simulation(1)
        points = max(points, int(_assert_same(a, b, f"step {s}")["num_points"].sum()))
    assert points > 0, "the scene made no contact point"
    return a, b


def test_box_pile():
    _lockstep(scenes.box_pile(8, 8, 8))


def test_mixed_box_sphere_pile():
    _lockstep(scenes.box_pile(8, 8, 8, mixed=True))


def test_capsule_ragdolls_with_joints():
    sc = scenes.figures(scenes.load_figure(os.path.join(GOLDEN, "ragdoll_capsule.npz")), 3, 2, pitch=1.0, ny=3, pitch_v=1.9)
    assert (sc["shape_type"] == scenes.SHAPE_CAPSULE).any()
    _lockstep(sc)


def test_polyhedron_heap_has_both_buckets_in_one_world():
    """Polyhedra and cylinders (staged kernels + k_np_merge on their manifolds alone) among boxes, spheres and capsules (k_np_contacts)."""
    from test_reference_engine import _polyhedron_scene
    sc = _polyhedron_scene()
    a, _ = _lockstep(sc)
    m = a.get_manifolds()
    m = m[m["num_points"] > 0]
    st = np.asarray(sc["shape_type"])[m["body"]]
    staged = np.isin(st, (scenes.SHAPE_POLYHEDRON, scenes.SHAPE_CYLINDER)).any(axis=1)
    assert staged.any() and (~staged).any(), "touching manifolds in both buckets"


def test_sleeping_pile_with_contact_events():
    """Island sleeping on: the sleeping-edge early-out of both phases, the copy of a sleeping manifold's points out of the previous
    array, and the contact events with their prefetched copy - through collapse, sleep and the steps after it."""
    scene = scenes.box_pile(3, 3, 3)
    a, b = _world(scene, True, sleeping=True, contact_events=True), _world(scene, False, sleeping=True, contact_events=True)
    a.set_event_prefetch(4096); b.set_event_prefetch(4096)
    asleep_since = None
    for s in range(1, 1201):
        a.step_simulation(1); b.step_simulation(1)
        _assert_same(a, b, f"step {s}")
        ea, eb = a.get_contact_events(), b.get_contact_events()   # lanes append with an atomic counter: the order within a step is free
        assert np.array_equal(_sorted_events(ea), _sorted_events(eb)), s
        (pa, ta), (pb, tb) = a.prefetched_events(), b.prefetched_events()
        assert ta == tb == len(ea) and np.array_equal(_sorted_events(pa), _sorted_events(pb)), s
        assert np.array_equal(a.get_point_ids(), b.get_point_ids()), s
        assert np.array_equal(a.get_asleep(), b.get_asleep()), s
        if asleep_since is None and a.get_asleep().any():
            asleep_since = s
        if asleep_since is not None and s >= asleep_since + 30:
            break
    assert asleep_since is not None, "the pile did not fall asleep"
