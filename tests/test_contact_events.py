"""Contact events under island sleeping, against the CPU oracle.

tests/test_gpu_parity.py holds the event list and the point ids to the oracle with sleeping off. Here sleeping is on, and the calls
take several steps, so that a call can put every island to sleep part way through and skip the steps that remain. After every call
the device's event list, the prefetched copy of it (edynhip_set_event_prefetch / edynhip_prefetched_events), the point ids and the
sleeping flags are compared with the oracle's.
"""
import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from oracle import binding as ob

from contact_scenes import DT_EXACT, MANIFOLD_CREATED, gap_touching_as_all_sleep, slide_scene

pytestmark = pytest.mark.gpu


def _sorted_events(ev):
    return np.sort(ev, order=["step", "type", "body", "point_id"])


def _worlds(scene, max_bodies=0, dt=1.0 / 60.0):
    g = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, sleeping=True,
                                            contact_events=True, max_bodies=max_bodies, fixed_dt=dt))
    g.set_scene(scene)
    o = ob.World(dt=dt, vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(scene)
    o.set_sleeping(True)
    o.record_events(True)
    return g, o


def _check_call(g, o, cap, what):
    """The events of the last call on both sides, the prefetched copy, the point ids and the sleeping flags. Returns the events."""
    eg, eo = g.get_contact_events(), o.get_events()
    o.clear_events()
    assert len(eg) == len(eo), (what, len(eg), len(eo))
    assert np.array_equal(_sorted_events(eg), _sorted_events(eo)), what
    early, total = g.prefetched_events()
    assert total == len(eg), (what, total, len(eg))
    assert len(early) == min(total, cap), (what, len(early), total, cap)
    if total <= cap:
        assert np.array_equal(_sorted_events(early), _sorted_events(eg)), what
    else:   # cut at the cap: the first events of the list, the true total reported
        assert np.array_equal(early, eg[:cap]), what
    assert np.array_equal(g.get_point_ids(), o.get_point_ids()), what
    assert np.array_equal(g.get_asleep(), o.get_asleep()), what
    return eg


def _dropped_box(x, y, z):
    s = scenes._empty(1)
    s["kind"][0] = scenes.KIND_DYNAMIC
    s["shape_type"][0] = scenes.SHAPE_BOX
    s["shape_param"][0, :3] = 0.5
    s["pos"][0] = (x, y, z)
    for k in ("inertia", "has_inertia", "joints"):
        s.pop(k)
    return s


@pytest.mark.parametrize("cap", [4096, 8])
def test_events_and_prefetch_through_collapse_sleep_and_wake(cap):
    """A 3x3x3 pile collapses and falls asleep in calls of 1, 2 and 3 steps, stays asleep for a while (calls that run no step),
    is woken by a box dropped on it and falls asleep again. Every call: events, prefetched events, point ids and sleeping flags
    as the oracle has them. cap=8: the prefetch is cut, the rest of the list is read from the device."""
    scene = scenes.box_pile(3, 3, 3)
    g, o = _worlds(scene, max_bodies=32)
    g.set_event_prefetch(cap)
    phase, calls_asleep, call, seen = "settle", 0, 0, 0
    phases = []
    while phase != "done":
        assert call < 1200, ("the pile did not sleep", phase)
        k = 1 + call % 3
        g.step_simulation(k); o.step(k)
        seen += len(_check_call(g, o, cap, (phase, call)))
        call += 1
        all_asleep = bool(g.get_asleep()[1:].all())
        if phase == "settle" and all_asleep:
            phase = "asleep"; phases.append(phase)
        elif phase == "asleep":
            assert all_asleep, call
            calls_asleep += 1
            if calls_asleep == 20:
                top = float(scene["pos"][1:, 1].max())
                box = _dropped_box(float(scene["pos"][1:, 0].mean()) + 0.1, top + 3.0, float(scene["pos"][1:, 2].mean()))
                g.add_scene(box); o.add_bodies(box)
                phase = "dropped"; phases.append(phase)
        elif phase == "dropped" and not g.get_asleep()[1:28].all():
            phase = "woken"; phases.append(phase)
        elif phase == "woken" and all_asleep:
            phase = "done"; phases.append(phase)
    assert phases == ["asleep", "dropped", "woken", "done"], phases
    assert seen > 300, seen


@pytest.mark.parametrize("timed", [False, True])
def test_prefetch_keeps_the_events_of_a_call_whose_last_step_is_skipped(timed):
    """Two-step calls; in the first step of one call box 2 touches box 1 and every island falls asleep, so the second step is
    skipped. The prefetched events of that call must still hold the (1, 2) MANIFOLD_CREATED, as the device's list and the
    oracle do. timed: the same through edynhip_step_timed (the max_steps_per_update clamp's path), with 1/64 s steps."""
    dt = DT_EXACT if timed else 1.0 / 60.0
    gap, step = gap_touching_as_all_sleep(dt, timed)
    assert gap is not None, "no gap makes the contact and the sleep fall into the same step"
    g, o = _worlds(slide_scene(gap), dt=dt)
    g.set_event_prefetch(64)
    done, hit = 0, False
    plan = [1] * (step % 2) + [2] * (step // 2 + 2)   # step (0-based) is the first of a two-step call
    for n in plan:
        if timed:   # stamps k * dt, as the search had them
            g.step_timed(n, done * dt, dt); o.step_timed(n, done * dt, dt)
        else:
            g.step_simulation(n); o.step(n)
        eg = _check_call(g, o, 64, (gap, done, n))
        if done == step:
            assert n == 2 and g.get_asleep()[1:].all()
            early, total = g.prefetched_events()
            mine = [e for e in early if e["type"] == MANIFOLD_CREATED and sorted(e["body"]) == [1, 2]]
            assert len(mine) == 1 and int(mine[0]["step"]) == step, (early, eg)
            hit = True
        done += n
    assert hit
