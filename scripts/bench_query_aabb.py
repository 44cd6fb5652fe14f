"""AABB query throughput on the device: 2^20 boxes of three sizes - a body's size, ten times that, and a box that covers 1 % of the
scene's volume - on the settled headline pile, mixed32k and the 262 144-box islands scene. Per scene and size: the query tree
(edynhip_query_aabb_device, count + scan + fill, boxes and result on the device), brute force (EDYNHIP_QUERY_BRUTE_FORCE, on a slice of
the boxes) and "download the AABBs and intersect in numpy" (edynhip_get_derived + tests/query_ref.py, on a smaller slice); queries/s and
hits/s each. Prints one JSON line.

    python scripts/bench_query_aabb.py [--boxes N] [--reps R] [--scenes pile32k,mixed32k,islands256k] [--ratios 4,16,64]

--ratios times the tree once per value of EDYNHIP_QUERY_SCAN_RATIO (a query that reports more than bodies / ratio hits is packed by a
wave striding the body range instead of written by its lane and sorted): the measurement behind the constant in query_aabb.hip.
Timing: device events around R calls after a warm-up call, on the context's stream.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import edyn_amd  # noqa: E402
from edyn_amd import scenes  # noqa: E402
import query_ref  # noqa: E402

SCENES = {"pile32k": (scenes.headline_pile, 300), "mixed32k": (lambda: scenes.box_pile(32, 32, 32, mixed=True), 120),
          "islands256k": (scenes.c4_islands, 120)}


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def boxes_of(n, lo, hi, half, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(lo, hi, size=(n, 3))
    return np.concatenate([c - half, c + half], axis=1).astype(np.float32)


def device_run(w, q, reps, dev, brute=False, category="procedural"):
    """(ms per call, total hits) of count + scan + fill with the ids buffer sized by a first, count-only call."""
    n = len(q)
    b = torch.zeros((2 * n, 4), dtype=torch.float32, device=dev)
    b[:, :3] = torch.from_numpy(q.reshape(-1, 3)).to(dev)
    off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    w.query_aabb_device(n, b.data_ptr(), off.data_ptr(), 0, 0, total.data_ptr(), category=category, brute_force=brute)
    w.synchronize()
    hits = int(total.cpu().numpy().view(np.uint32)[0])
    ids = torch.zeros(max(hits, 1), dtype=torch.int32, device=dev)
    call = lambda: w.query_aabb_device(n, b.data_ptr(), off.data_ptr(), ids.data_ptr(), hits, total.data_ptr(), category=category, brute_force=brute)  # noqa: E731
    call()
    return timed(call, reps), hits


def rate(n, hits, ms):
    return {"ms": round(ms, 4), "queries_per_s": round(n / (ms * 1e-3)), "hits_per_s": round(hits / (ms * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="pile32k,mixed32k,islands256k")
    ap.add_argument("--ratios", default="", help="comma-separated EDYNHIP_QUERY_SCAN_RATIO values to time the tree with (default: the built-in one only)")
    ap.add_argument("--brute-boxes", type=int, default=1 << 14)
    ap.add_argument("--numpy-boxes", type=int, default=1 << 10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ratios = [int(r) for r in a.ratios.split(",") if r] or [None]
    result = {"boxes": a.boxes, "reps": a.reps, "scenes": {}}
    for name in a.scenes.split(","):
        gen, settle = SCENES[name]
        scene = gen()
        per_ratio = {}
        for ratio in ratios:
            if ratio is None:
                os.environ.pop("EDYNHIP_QUERY_SCAN_RATIO", None)
            else:
                os.environ["EDYNHIP_QUERY_SCAN_RATIO"] = str(ratio)
            w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3))
            w.set_scene(scene)
            stream = torch.cuda.Stream()
            w.set_stream(stream.cuda_stream)
            torch.cuda.set_stream(stream)
            w.step_simulation(settle)
            aabb = w.get_derived()[0]
            body = (scene["shape_type"] != scenes.SHAPE_PLANE) & (scene["shape_type"] != scenes.SHAPE_NONE)
            lo, hi = aabb[body, :3].min(0), aabb[body, 3:].max(0)
            size = float(np.median(aabb[body, 3:] - aabb[body, :3])) * 0.5
            sizes = {"body": size, "10x": 10 * size, "1pct": 0.5 * float(np.prod(hi - lo) * 0.01) ** (1.0 / 3.0)}
            out = {"bodies": int(len(scene["kind"]))}
            for label, half in sizes.items():
                q = boxes_of(a.boxes, lo, hi, half, 1)
                while True:   # (a result beyond 2^32 - 1 ids: halve the batch)
                    ms, hits = device_run(w, q, a.reps, dev)
                    if hits < 0xFFFFFFFF:
                        break
                    q = q[:len(q) // 2]
                row = {"half_extent": round(half, 3), "boxes": len(q), "hits_per_query": round(hits / len(q), 2), "tree": rate(len(q), hits, ms),
                       "wave_paths": list(w.query_aabb_stats())}
                if ratio is ratios[0]:
                    qb = q[:a.brute_boxes]
                    ms_b, hits_b = device_run(w, qb, max(1, a.reps // 2), dev, brute=True)
                    row["brute_force"] = dict(rate(len(qb), hits_b, ms_b), boxes=len(qb))
                    qn = q[:a.numpy_boxes]
                    dyn = body & (scene["kind"] == scenes.KIND_DYNAMIC)
                    t = time.perf_counter()
                    boxes_host = w.get_derived()[0]
                    off, ids = query_ref.query(boxes_host[dyn], qn, ids=np.flatnonzero(dyn))
                    dt = (time.perf_counter() - t) * 1e3
                    row["numpy_on_host"] = dict(rate(len(qn), int(off[-1]), dt), boxes=len(qn))
                out[label] = row
            if name == "islands256k" and ratio is ratios[0]:
                q = boxes_of(a.boxes, lo, hi, sizes["10x"], 2)
                ms, hits = device_run(w, q, a.reps, dev, category="islands")
                out["islands_10x"] = dict(rate(len(q), hits, ms), hits_per_query=round(hits / len(q), 2))
            per_ratio["default" if ratio is None else str(ratio)] = out
            del w
        result["scenes"][name] = per_ratio
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
