"""What an edit of ONE body of a running multi-device world costs through edynhip_world_edit_bodies: on the settled islands scene
(scenes.c4_islands(), 262 144 boxes in 4 096 mini-piles) with 2 and 8 shards, ALL ON DEVICE 0, per field group the median wall time of

    edit+step  MultiWorld.edit_bodies of one box in a pile, then one step;
    call       the call alone (it returns when the shards hold the edit and the world's tables follow);
    former     the route every such edit took before: the whole scene described again with the current state and the edited body
               (set_scene), every shard built (get_partition), one step - measured in the same process, alternating with the edit.

Groups: mass, inertia, material, shape, kind within a class (the plane static <-> kinematic), and the two crossing edits - a pile box made
static, and made dynamic again - which rebuild every shard but the owner; for those the full re-partition of the same world
(MultiWorld.repartition, every shard rebuilt through the same carry) is timed beside them.

    python scripts/bench_world_body_edits.py [--scene islands256k|piles4k] [--shards 2,8] [--reps 5] [--out profiles/world_body_edits.json]

The script checks the structural claim through the edit statistics: the non-crossing edits ran in place, no shard rebuilt, no
re-partition. Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import edyn_amd  # noqa: E402
from edyn_amd import scenes  # noqa: E402
from edyn_amd.multi import MultiWorld  # noqa: E402

SCENES = {"islands256k": scenes.c4_islands, "piles4k": lambda: scenes.mini_piles(8, 8)}
I_NEW = np.diag([0.3, 0.25, 0.35]).astype(np.float32).reshape(9)
DYN, KIN, STA = scenes.KIND_DYNAMIC, scenes.KIND_KINEMATIC, scenes.KIND_STATIC


def edits_of(k, n):
    """(group, body, keyword arguments of edit_bodies) for repetition k: a box inside another pile each time."""
    body = 1 + 64 * ((17 * k + 3) % ((n - 1) // 64)) + 21
    return [("mass", body, dict(mass=[2.0 + k])),
            ("inertia", body, dict(inertia=[I_NEW * (1 + k)])),
            ("material", body, dict(friction=[0.3 + 0.05 * k], restitution=[0.0])),
            ("shape", body, dict(shape_type=[scenes.SHAPE_SPHERE if k % 2 == 0 else scenes.SHAPE_BOX], shape_param=[(0.5, 0.5 * (k % 2), 0.5 * (k % 2), 0)])),
            ("kind_in_class", 0, dict(kind=[KIN if k % 2 == 0 else STA])),
            ("cross_to_static", body + 1, dict(kind=[STA])),
            ("cross_to_dynamic", body + 1, dict(kind=[DYN], mass=[1.0], inertia=[I_NEW]))]


def describe(desc, body, kw):
    """The edit applied to the scene description the former route uploads."""
    if "mass" in kw:
        desc["mass"][body] = kw["mass"][0]
    if "inertia" in kw:
        desc["inertia"][body] = kw["inertia"][0]; desc["has_inertia"][body] = 1
    if "friction" in kw:
        desc["friction"][body] = kw["friction"][0]; desc["restitution"][body] = kw["restitution"][0]
    if "shape_type" in kw:
        desc["shape_type"][body] = kw["shape_type"][0]; desc["shape_param"][body] = kw["shape_param"][0]
    if "kind" in kw:
        desc["kind"][body] = kw["kind"][0]


def run(scene, shards, reps, warm):
    mw = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10), devices=[0] * shards)
    desc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    mw.set_scene(desc)
    mw.step_simulation(warm)
    n = mw.n
    names = [g for g, _, _ in edits_of(0, n)]
    t_edit, t_call, t_former, t_full = ({g: [] for g in names} for _ in range(4))
    crossing = ("cross_to_static", "cross_to_dynamic")

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter(); fn(); return (time.perf_counter() - t) * 1e3

    for k in range(reps):
        for group, body, kw in edits_of(k, n):
            before = mw.get_edit_stats()
            call = clock(lambda: mw.edit_bodies([body], **kw))
            step = clock(lambda: mw.step_simulation(1))
            st = mw.get_edit_stats()
            if group not in crossing:
                assert st["in_place"] == before["in_place"] + 1 and st["shard_rebuilds"] == before["shard_rebuilds"] and \
                    st["repartitions_by_edit"] == before["repartitions_by_edit"], (group, st)
            else:
                assert st["shard_rebuilds"] == before["shard_rebuilds"] + shards - 1, (group, st)
                t_full[group].append(clock(lambda: (mw.repartition(), mw.step_simulation(1))))
            t_call[group].append(call); t_edit[group].append(call + step)
            describe(desc, body, kw)
            # the former route, alternating: the same world described again with the current state and the edited body
            for key, a in zip(("pos", "orn", "linvel", "angvel"), mw.get_state()):
                desc[key] = a.copy()
            t_former[group].append(clock(lambda: (mw.set_scene(desc), mw.get_partition(), mw.step_simulation(1))))
    mw.close()
    med = statistics.median
    out = {"shards": shards, "bodies": int(n), "groups": {}}
    for g in names:
        row = {"edit_plus_step_ms": round(med(t_edit[g]), 3), "call_ms": round(med(t_call[g]), 3), "former_route_ms": round(med(t_former[g]), 1),
               "former_over_edit": round(med(t_former[g]) / med(t_edit[g]), 1), "edit_plus_step_ms_all": [round(x, 3) for x in t_edit[g]],
               "former_route_ms_all": [round(x, 1) for x in t_former[g]]}
        if g in crossing:
            row["full_repartition_plus_step_ms"] = round(med(t_full[g]), 1)
        out["groups"][g] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="islands256k", choices=sorted(SCENES))
    ap.add_argument("--shards", default="2,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_body_edits.json"))
    a = ap.parse_args()
    scene = SCENES[a.scene]()
    res = {"bench": "world_body_edits", "scene": a.scene, "device": torch.cuda.get_device_name(0), "placement": "one GPU, every shard on device 0", "reps": a.reps,
           "what": "median wall ms per field group: one body edited through edynhip_world_edit_bodies plus the next step / the call alone / the former route "
                   "(set_scene with the current state, build, one step) in the same process, alternating; crossing edits beside a full re-partition plus a step",
           "runs": [run(scene, int(s), a.reps, a.warm) for s in a.shards.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
