"""What an edit of a body of a running world costs: on the settled headline pile (scenes.headline_pile(), 32 768 boxes) and on
scenes.box_pile(6, 6, 6), per field group of edynhip_edit_bodies (mass, inertia, material, shape, kind), the median wall time of

    in_place  World.edit_bodies of ONE body plus the next step (edit_call: the call alone);
    rebuild   what the same edit cost before the call existed, built from public calls: read the manifolds, the joint impulses, the
              sleeping flags and timers; destroy the context, create one, set_scene with the edited description at the current state;
              set_manifolds (without the edited body's manifolds for shape / kind) and the rest; the next step.

    python scripts/bench_body_edits.py [--scenes headline,pile216] [--reps 7] [--out profiles/body_edits_bench.json]

Both are timed in one process, alternating, the wall clock around calls that end with a synchronize; every repetition edits another
body of the pile's top layers, and both worlds take the same edits. Two more figures per scene: the steady-state step of a world after
a MASS edit beside the same step of an untouched copy (alternating batches of steps; the copy's own run-to-run spread is the yardstick),
and whether the edited world went on over the same code paths as the copy (candidate lists kept, manifold array kept in place: the
debug-path sets agree). Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import edyn_amd  # noqa: E402
from edyn_amd import scenes  # noqa: E402

SCENES = {"headline": (scenes.headline_pile, 120), "pile216": (lambda: scenes.box_pile(6, 6, 6), 60)}
GROUPS = ("mass", "inertia", "material", "shape", "kind")
KIN, DYN = 1, scenes.KIND_DYNAMIC
I_NEW = np.diag([0.3, 0.25, 0.2]).astype(np.float32).reshape(9)


def explicit_inertia(scene):
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    need = (s["kind"] == DYN) & (s["has_inertia"] == 0)
    s["inertia"][need] = np.outer(s["mass"][need] / np.float32(6), np.eye(3, dtype=np.float32).reshape(9))
    s["has_inertia"][need] = 1
    return s


def make_world(scene):
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3))
    w.set_scene(scene)
    return w


def the_edit(group, body):
    if group == "mass":
        return dict(mass=[2.5])
    if group == "inertia":
        return dict(inertia=[I_NEW])
    if group == "material":
        return dict(friction=[0.8])
    if group == "shape":
        return dict(shape_type=[scenes.SHAPE_SPHERE], shape_param=[(0.5, 0, 0, 0)])
    return dict(kind=[KIN])


def describe(scene, body, kw):
    """The description after the edit (the scene's arrays are edited in place: both worlds share the description)."""
    for k in ("mass", "friction", "kind", "shape_type"):
        if k in kw:
            scene[k][body] = kw[k][0]
    if "inertia" in kw:
        scene["inertia"][body] = kw["inertia"][0]
    if "shape_param" in kw:
        scene["shape_param"][body] = kw["shape_param"][0]


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def rebuild(w, scene, body, group):
    """The route from before the call, as the C++ drop-in took it. Returns the new world."""
    m = w.get_manifolds()
    mine = (m["body"][:, 0] == body) | (m["body"][:, 1] == body)
    if group in ("shape", "kind"):
        m = m[~mine]
    elif group == "material":   # the carried points of the body take the mixed friction of the current materials (no mix table here)
        other = np.where(m["body"][mine, 0] == body, m["body"][mine, 1], m["body"][mine, 0])
        mixed = np.sqrt(scene["friction"][body] * scene["friction"][other]).astype(np.float32)
        fr = m["pt"]["friction"]
        fr[mine] = mixed[:, None]
        m["pt"]["friction"] = fr
    state = w.get_state()
    w.get_joint_impulses24(); w.get_asleep(); w.get_sleep_timers()   # (read as the shim reads them; this scene has neither joints nor sleepers)
    w.detach()
    s = dict(scene)
    s["pos"], s["orn"], s["linvel"], s["angvel"] = state
    n = make_world(s)
    n.set_manifolds(m)
    n.step_simulation(1)
    n.synchronize()
    return n


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs) if xs else 0.0


def run(name, reps):
    gen, settle = SCENES[name]
    scene = explicit_inertia(gen())
    a, b = make_world(scene), make_world(scene)
    a.step_simulation(settle); b.step_simulation(settle)
    a.synchronize(); b.synchronize()
    n = len(scene["kind"])
    out = {"bodies": n, "manifolds": int(len(a.get_manifolds())), "groups": {}}
    body = n - 1
    for group in GROUPS:
        ta, tb, te = [], [], []
        for _ in range(reps):
            body -= 1
            kw = the_edit(group, body)
            describe(scene, body, kw)

            def the_call():
                a.edit_bodies([body], **kw)
                a.synchronize()

            def the_step():
                a.step_simulation(1)
                a.synchronize()
            te.append(timed(the_call))
            ta.append(te[-1] + timed(the_step))
            holder = {}
            tb.append(timed(lambda: holder.setdefault("w", rebuild(b, scene, body, group))))
            b = holder["w"]
        same = all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state()))
        out["groups"][group] = {"edit_call_ms": statistics.median(te), "in_place_ms": statistics.median(ta), "rebuild_ms": statistics.median(tb), "ratio": statistics.median(tb) / statistics.median(ta),
                                "in_place_all_ms": ta, "rebuild_all_ms": tb, "rebuild_spread": spread(tb), "same_state_after": bool(same)}
    # the steady-state step after a MASS edit beside an untouched copy (two fresh worlds, settled alike)
    c, d = make_world(scene), make_world(scene)
    c.step_simulation(settle); d.step_simulation(settle)
    c.edit_bodies([n - 2], mass=[float(scene["mass"][n - 2])])   # (the value it has: the two go on alike, only the call differs)
    batch, tc, td = 50, [], []
    for _ in range(max(reps, 5)):
        def steps(w):
            w.step_simulation(batch)
            w.synchronize()
        tc.append(timed(lambda: steps(c)) / batch)
        td.append(timed(lambda: steps(d)) / batch)
    out["step_after_mass_edit_ms"] = statistics.median(tc)
    out["step_untouched_ms"] = statistics.median(td)
    out["step_untouched_spread"] = spread(td)
    out["step_excess"] = statistics.median(tc) / statistics.median(td) - 1.0
    out["same_paths_as_untouched"] = c.debug_paths() == d.debug_paths()
    out["paths"] = sorted(c.debug_paths())
    for w in (a, b, c, d):
        w.detach()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="headline,pile216")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_edits_bench.json"))
    args = ap.parse_args()
    result = {"bench": "body_edits", "reps": args.reps, "scenes": {name: run(name, max(args.reps, 5)) for name in args.scenes.split(",")}}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
