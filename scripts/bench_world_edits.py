"""What an edit of a running multi-device world costs: on the settled islands scene (scenes.c4_islands(), 262 144 boxes in 4 096
mini-piles) with 2 and 8 shards, ALL ON DEVICE 0, the median wall time of

    spawn    one mini-pile (64 boxes, one MultiWorld.add_scene call) next to the field - in place on one shard;
    remove   one body (MultiWorld.remove_bodies) - in place on its shard;
    rebuild  the route every edit took before the world could be edited: describe the whole scene again with the current state
             (set_scene) and let the next call build every shard - measured in the same run, on the same world size.

    python scripts/bench_world_edits.py [--scene islands256k|piles4k] [--shards 2,8] [--reps 7] [--rebuild-reps 3] [--out profiles/world_edits.json]

Every edit call is synchronous (it returns when the shards hold the edit and the world's tables follow), so the wall clock around the
call is the cost; the rebuild is timed around set_scene + get_partition (which builds the shards, as the next step would; set_scene's
own conversion of the scene's arrays is inside the window, assembling the scene with the current state is not). The script
also checks the structural claim through the edit statistics: no shard rebuilt, no re-partition. Prints one JSON line and writes it to --out.
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

import torch  # noqa: E402

import edyn_amd  # noqa: E402
from edyn_amd import scenes  # noqa: E402
from edyn_amd.multi import MultiWorld  # noqa: E402

SCENES = {"islands256k": (scenes.c4_islands, 64), "piles4k": (lambda: scenes.mini_piles(8, 8), 8)}


def one_pile(x, z):
    """A mini-pile of its own at (x, z): the 64 boxes of scenes.mini_piles(1, 1) without the floor."""
    s = scenes.subset(scenes.mini_piles(1, 1), np.arange(1, 65))
    s["pos"][:, 0] += np.float32(x); s["pos"][:, 2] += np.float32(z)
    return s


def with_state(scene, n0, extra, state):
    """The scene as it is now: the first bodies plus the piles spawned since, at the current state."""
    out = {k: (np.concatenate([v] + [e[k] for e in extra]) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    for k, a in zip(("pos", "orn", "linvel", "angvel"), state):
        out[k] = a.copy()
    return out


def run(scene, sites_x, shards, reps, rebuild_reps, warm):
    mw = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10), devices=[0] * shards)
    mw.set_scene(scene)
    mw.step_simulation(warm)
    n0 = mw.n
    edge = (sites_x / 2.0 + 1.0) * 8.0
    spawn, remove, rebuild, extra = [], [], [], []
    for k in range(reps):
        pile = one_pile(edge + 8.0 * k, 0.0)
        torch.cuda.synchronize()
        t = time.perf_counter(); mw.add_scene(pile); spawn.append((time.perf_counter() - t) * 1e3)
        extra.append(pile)
        mw.step_simulation(2)
    for k in range(reps):
        victim = 1 + 64 * ((17 * k + 3) % (n0 // 64)) + 63
        torch.cuda.synchronize()
        t = time.perf_counter(); mw.remove_bodies([victim]); remove.append((time.perf_counter() - t) * 1e3)
        mw.step_simulation(2)
    st = mw.get_edit_stats()
    assert st["shard_rebuilds"] == 0 and st["repartitions_by_edit"] == 0 and st["in_place"] == st["edits"] == 2 * reps, st
    for k in range(rebuild_reps):
        now = with_state(scene, n0, extra, mw.get_state())
        torch.cuda.synchronize()
        t = time.perf_counter(); mw.set_scene(now); mw.get_partition(); rebuild.append((time.perf_counter() - t) * 1e3)
        mw.step_simulation(2)
    mw.close()
    med = statistics.median
    return {"shards": shards, "bodies": int(n0), "spawn_pile_ms": round(med(spawn), 3), "remove_body_ms": round(med(remove), 3),
            "rebuild_ms": round(med(rebuild), 1), "spawn_ms_all": [round(x, 3) for x in spawn], "remove_ms_all": [round(x, 3) for x in remove],
            "rebuild_ms_all": [round(x, 1) for x in rebuild], "edit_stats": st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="islands256k", choices=sorted(SCENES))
    ap.add_argument("--shards", default="2,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_edits.json"))
    a = ap.parse_args()
    make, sites_x = SCENES[a.scene]
    scene = make()
    res = {"bench": "world_edits", "scene": a.scene, "device": torch.cuda.get_device_name(0), "placement": "one GPU, every shard on device 0", "reps": a.reps, "rebuild_reps": a.rebuild_reps,
           "what": "median wall ms: one 64-box mini-pile spawned in place / one body removed in place / the whole scene described again with the current state and rebuilt",
           "runs": [run(scene, sites_x, int(s), a.reps, a.rebuild_reps, a.warm) for s in a.shards.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
