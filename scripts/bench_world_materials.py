"""What a re-partition of a multi-device world costs when the contact points' extras travel with it (materials on a multi-device world).

On the settled islands scene (scenes.c4_islands(), 262 144 boxes in 4 096 mini-piles; --scene piles4k for a small one), 2 shards ON
DEVICE 0, one run = one fresh process that builds the world, steps it `--warm` times and takes the median wall time of `--reps` forced
re-partitions (MultiWorld.repartition: every shard is read in full and rebuilt - what a meeting of two islands costs the shards it
touches, here all of them), a step between two of them. The call is synchronous, so the wall clock around it is the cost.

    python scripts/bench_world_materials.py [--scene islands256k] [--runs 5] [--parent-root PATH] [--out profiles/world_materials_meeting.json]

  with materials     rolling and spinning friction on the ground and every box: every point has extras rows, all are carried
  without materials  nothing is gathered, copied or allocated for extras (edynhip_world_stats.extras_carries stays 0)
  --parent-root      a checkout of the parent commit with its library built: the run without materials alternates between the two
                     trees, `--runs` processes each, and the medians are compared with the parent's own spread (max - min of its runs)

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, a.root or ROOT)
    import numpy as np
    import torch
    import edyn_amd
    from edyn_amd import scenes
    from edyn_amd.multi import MultiWorld
    scene = scenes.c4_islands() if a.scene == "islands256k" else scenes.mini_piles(8, 8)
    mw = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10), devices=[0] * a.shards)
    mw.set_scene(scene)
    if a.materials:
        n = len(scene["kind"])
        mw.set_material_extras(0, spin=np.full(n, 0.03, np.float32), roll=np.full(n, 0.02, np.float32))
    mw.step_simulation(a.warm)
    ms = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter(); mw.repartition(); ms.append((time.perf_counter() - t) * 1e3)
        mw.step_simulation(1)
    st = mw.get_stats()
    carried = st.get("extras_carries", 0)
    if "extras_carries" in st:
        assert carried == (a.reps if a.materials else 0), st
    print(json.dumps({"materials": bool(a.materials), "repartition_ms": round(statistics.median(ms), 2), "all_ms": [round(x, 2) for x in ms],
                      "manifolds": int(len(mw.get_manifolds())), "bodies": int(mw.n)}))
    mw.close()


def run_child(a, materials, root=None):
    env = dict(os.environ)
    env.pop("EDYNHIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(root or ROOT), "--scene", a.scene, "--shards", str(a.shards), "--warm", str(a.warm), "--reps", str(a.reps)]
    out = subprocess.run(cmd + (["--materials"] if materials else []), env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(out.stdout + out.stderr)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="islands256k", choices=["islands256k", "piles4k"])
    ap.add_argument("--shards", type=int, default=2)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--materials", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_materials_meeting.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    med = statistics.median
    res = {"bench": "world_materials_meeting", "scene": a.scene, "shards": a.shards, "device": torch.cuda.get_device_name(0), "placement": "one GPU, every shard on device 0",
           "what": "wall ms of one forced full re-partition (every shard read in full and rebuilt); per run the median of %d, per variant the median of %d runs (fresh processes)" % (a.reps, a.runs)}
    plain, parent = [], []
    for _ in range(a.runs):     # alternating: parent, this commit, parent, ...
        if a.parent_root:
            parent.append(run_child(a, False, a.parent_root))
        plain.append(run_child(a, False))
    withm = [run_child(a, True) for _ in range(a.runs)]
    res["bodies"], res["manifolds"] = plain[0]["bodies"], plain[0]["manifolds"]
    res["with_materials_ms"] = med(r["repartition_ms"] for r in withm); res["with_materials_runs"] = [r["repartition_ms"] for r in withm]
    res["without_materials_ms"] = med(r["repartition_ms"] for r in plain); res["without_materials_runs"] = [r["repartition_ms"] for r in plain]
    res["carry_cost_ms"] = round(res["with_materials_ms"] - res["without_materials_ms"], 2)
    res["carried_bytes"] = 128 * withm[0]["manifolds"]
    if parent:
        runs = [r["repartition_ms"] for r in parent]
        res["parent_without_materials_ms"] = med(runs); res["parent_runs"] = runs
        res["parent_spread_ms"] = round(max(runs) - min(runs), 2)
        res["over_parent_ms"] = round(res["without_materials_ms"] - res["parent_without_materials_ms"], 2)
        res["within_parent_spread"] = bool(res["over_parent_ms"] <= res["parent_spread_ms"])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
