"""Scenes for the contact-event tests (tests/test_contact_events.py, tests/cpp/contact_mirror.cpp through test_cpp_shim.py), and the
oracle searches that place them: where a contact and a put-to-sleep fall into the same step depends on every rounding of the solve,
so it is found with the CPU oracle at run time rather than written down."""
import numpy as np

from edyn_amd import scenes
from oracle import binding as ob

MANIFOLD_CREATED = 1
DT_EXACT = 1.0 / 64   # a step length whose multiples are exact: timed stamps k * dt do not depend on how steps are grouped into calls


def slide_scene(gap):
    """A plane and two frictionless unit boxes: box 1 rests at x = 0, box 2 rests at x = 1 + gap and slides towards it slower
    than the sleep threshold (0.005), so that it may touch box 1 in the very step after which every body is asleep."""
    s = scenes._empty(3)
    scenes._add_plane(s)
    s["shape_type"][1:] = scenes.SHAPE_BOX
    s["shape_param"][1:, :3] = 0.5
    s["pos"][1] = (0, 0.5, 0)
    s["pos"][2] = (1 + gap, 0.5, 0)
    s["linvel"][2] = (-0.004, 0, 0)
    s["friction"][:] = 0
    return s


def touch_and_sleep(gap, dt, timed, steps=200):
    """Oracle alone, one step at a time (10 velocity, 3 position iterations, sleeping on): (step that creates the (1, 2)
    manifold or None, step after which every dynamic body is asleep or None). timed: step k carries the stamp k * dt."""
    o = ob.World(dt=dt, vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(slide_scene(gap)); o.set_sleeping(True); o.record_events(True)
    created = None
    for k in range(steps):
        if timed:
            o.step_timed(1, k * dt, dt)
        else:
            o.step(1)
        for e in o.get_events():
            if created is None and e["type"] == MANIFOLD_CREATED and sorted(e["body"]) == [1, 2]:
                created = int(e["step"])
        o.clear_events()
        if o.get_asleep()[1:].all():
            return created, k
    return created, None


def gap_touching_as_all_sleep(dt, timed):
    """Bisect the gap of slide_scene until box 2's manifold is created in the step after which every body sleeps (a window a few
    1e-5 m wide). Returns (gap, step), or (None, None) when no such gap exists."""
    lo, hi = 0.02, 0.04   # touches long before every body sleeps / never touches before
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        created, asleep = touch_and_sleep(mid, dt, timed)
        if created is not None and created == asleep:
            return mid, created
        if created is not None and (asleep is None or created < asleep):
            lo = mid
        else:
            hi = mid
    return None, None


def landing_grid(n=32, pitch=2.0, drop=0.5):
    """n x n unit boxes, far enough apart never to touch, all dropped from the same height onto a plane: they land in the same
    step, which creates a manifold and four points per box. (tests/cpp/contact_mirror.cpp builds the same grid.)"""
    s = scenes._empty(n * n + 1)
    scenes._add_plane(s)
    s["shape_type"][1:] = scenes.SHAPE_BOX
    s["shape_param"][1:, :3] = 0.5
    i = np.arange(n * n)
    s["pos"][1:, 0] = pitch * (i % n)
    s["pos"][1:, 1] = 0.5 + drop
    s["pos"][1:, 2] = pitch * (i // n)
    return s


def most_events_in_one_step(scene, steps, vel_iters=8, pos_iters=3):
    """The oracle's largest number of contact events in a single step over the first `steps` steps."""
    o = ob.World(vel_iters=vel_iters, pos_iters=pos_iters, order=ob.ORDER_COLOURED)
    o.add_bodies(scene); o.set_sleeping(True); o.record_events(True)
    most = 0
    for _ in range(steps):
        o.step(1)
        most = max(most, len(o.get_events()))
        o.clear_events()
    return most
