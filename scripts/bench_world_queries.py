"""Queries on a multi-device world against the single-context calls: 1 048 576 random rays (lengths 0.5 to 50 m) and 1 048 576
body-sized boxes (category procedural) on the settled 262 144-box islands scene. The baseline is World.raycast_device /
World.query_aabb_device on one context; then a MultiWorld of 1, 2, 4 and 8 shards, ALL ON DEVICE 0 (what the shards add when they
share one GPU: several smaller traces instead of one, the index translation and the merge; on separate GPUs the traces run side by
side and the copies between devices come on top - not measured here). Prints one JSON line and writes it to --out.

    python scripts/bench_world_queries.py [--rays N] [--boxes N] [--reps R] [--shards 1,2,4,8] [--out profiles/world_queries.json]

The scene is settled on the single context; every world is described with that state and queried without a step of its own (a
described world answers for the described state), so all of them hold the same bodies at the same places and the script also checks
that every world returns the single context's bytes. Timing: wall clock around a window of R calls between device synchronisations,
after warm-up; the world's calls block until the answer is complete, the single context's are enqueued and the window ends with a
synchronisation. For where the time goes inside a call: `rocprofv3 --kernel-trace --stats -- python scripts/bench_world_queries.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import edyn_amd  # noqa: E402
from edyn_amd import scenes  # noqa: E402
from edyn_amd.multi import MultiWorld  # noqa: E402

SCENES = {"islands256k": (scenes.c4_islands, 120), "piles4k": (lambda: scenes.mini_piles(8, 8), 120)}


def rays(n, lo, hi, seed=1):
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return p0, (p0 + d * rng.uniform(0.5, 50.0, size=(n, 1))).astype(np.float32)


def boxes(n, aabb, seed=2):
    """The fat boxes' size: a randomly picked body's AABB moved by up to its own size."""
    rng = np.random.default_rng(seed)
    pick = aabb[rng.integers(0, len(aabb), n)]
    ext = pick[:, 3:] - pick[:, :3]
    shift = rng.uniform(-1, 1, size=(n, 3)) * ext
    return np.concatenate([pick[:, :3] + shift, pick[:, 3:] + shift], axis=1).astype(np.float32)


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def measure(world, nr, t0, t1, out, nb, tb, off, ids, total, capacity, reps):
    ray = lambda: world.raycast_device(nr, t0.data_ptr(), t1.data_ptr(), out.data_ptr())  # noqa: E731
    box = lambda: world.query_aabb_device(nb, tb.data_ptr(), off.data_ptr(), ids.data_ptr(), capacity, total.data_ptr())  # noqa: E731
    for _ in range(2):
        ray(); box()
    r = {"raycast_ms": round(timed(ray, reps), 4), "query_aabb_ms": round(timed(box, reps), 4)}
    torch.cuda.synchronize()
    return r, out.cpu().numpy().tobytes(), off.cpu().numpy().tobytes(), ids.cpu().numpy().tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--scene", default="islands256k", choices=sorted(SCENES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = lambda: edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3)  # noqa: E731
    gen, settle = SCENES[a.scene]
    scene = gen()
    single = edyn_amd.World(cfg())
    single.set_scene(scene)
    single.step_simulation(settle)
    pos, orn, lv, av = single.get_state()
    aabb, _, _ = single.get_derived()
    shaped = scene["shape_type"] != scenes.SHAPE_PLANE
    lo, hi = aabb[shaped, :3].min(0), aabb[shaped, 3:].max(0)
    p0, p1 = rays(a.rays, lo - 2, hi + 2)
    q = boxes(a.boxes, aabb[shaped])
    t0 = torch.zeros((a.rays, 4), dtype=torch.float32, device=dev); t0[:, :3] = torch.from_numpy(p0).to(dev)
    t1 = torch.zeros((a.rays, 4), dtype=torch.float32, device=dev); t1[:, :3] = torch.from_numpy(p1).to(dev)
    out = torch.zeros((a.rays, 8), dtype=torch.int32, device=dev)
    tb = torch.zeros((2 * a.boxes, 4), dtype=torch.float32, device=dev); tb[:, :3] = torch.from_numpy(q.reshape(-1, 3)).to(dev)
    off = torch.zeros(a.boxes + 1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    ids = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    single.query_aabb_device(a.boxes, tb.data_ptr(), off.data_ptr(), None, 0, total.data_ptr())
    single.synchronize()
    capacity = int(total.cpu().numpy().view(np.uint32)[0])
    ids = torch.zeros(max(capacity, 1), dtype=torch.int32, device=dev)
    base, *ref = measure(single, a.rays, t0, t1, out, a.boxes, tb, off, ids, total, capacity, a.reps)
    hits = np.frombuffer(ref[0], np.uint32).reshape(-1, 8)[:, 0]
    line = {"scene": a.scene, "bodies": int(len(scene["kind"])), "rays": a.rays, "boxes": a.boxes, "box_hits": capacity, "reps": a.reps,
            "ray_hit_fraction": round(float((hits != 0xFFFFFFFF).mean()), 4), "single_context": base, "world": {}}
    moved = dict(scene)   # the settled state as a scene description
    moved["pos"], moved["orn"], moved["linvel"], moved["angvel"] = pos, orn, lv, av
    for shards in [int(x) for x in a.shards.split(",")]:
        mw = MultiWorld(cfg(), devices=[0] * shards)
        mw.set_scene(moved)
        r, *got = measure(mw, a.rays, t0, t1, out, a.boxes, tb, off, ids, total, capacity, a.reps)
        r["equals_single_context"] = got == ref
        r["bodies_per_shard"] = mw.get_stats()["bodies_per_shard"]
        for k in ("raycast_ms", "query_aabb_ms"):
            r[k.replace("_ms", "_over_single")] = round(r[k] / base[k], 3)
        line["world"][str(shards)] = r
        mw.close()
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
