"""Raycast throughput on the device: query-tree build time and rays per second for 1 048 576 random rays (lengths 0.5 to 50 m)
on the headline pile (settled) and on the 262 144-box islands scene. Prints one JSON line per scene.

    python scripts/bench_raycast.py [--rays N] [--reps R] [--scenes pile32k,islands256k]

Timing: device events around a window of R raycast_device calls after warm-up (the rays and results stay on the device). The
build is timed as R x (refresh_derived, then a one-ray raycast, which rebuilds boxes and tree) minus R x refresh_derived minus
R x a one-ray raycast on a built tree. For where the time goes inside a call, run it under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_raycast.py`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import edyn_amd  # noqa: E402
from edyn_amd import scenes  # noqa: E402

SCENES = {"pile32k": (scenes.headline_pile, 300), "islands256k": (scenes.c4_islands, 120)}


def rays(n, lo, hi, seed=1):
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return p0, (p0 + d * rng.uniform(0.5, 50.0, size=(n, 1))).astype(np.float32)


def reference_baseline(w, scene, p0, p1, dev_hits):
    """CPU baseline: the reference's own edyn::raycast, single-threaded, over the first rays of the batch, on the device's state
    (the real engine built from the device's transforms in zero gravity with zero velocities and stepped once, so its trees hold
    the current AABBs). Returns rays/s and how many of those rays hit the same body as on the device."""
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_raycast as mr
    pos, orn, _, _ = w.get_state()
    s = dict(scene)
    s["pos"], s["orn"] = pos, orn
    s["linvel"] = np.zeros_like(pos); s["angvel"] = np.zeros_like(pos)
    r = mr.reference_world(s)
    t = time.perf_counter()
    res = mr.reference_raycast(r, p0, p1)
    dt = time.perf_counter() - t
    return {"what": "reference edyn::raycast, one CPU thread, ctypes call per ray (includes ~1 us of call overhead)",
            "rays": int(len(p0)), "rays_per_s": round(len(p0) / dt), "same_body_as_device": round(float((res["entity"] == dev_hits).mean()), 4)}


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", default="pile32k,islands256k")
    ap.add_argument("--cpu-rays", type=int, default=20000, help="rays for the reference's CPU baseline (0 = skip)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.scenes.split(","):
        gen, settle = SCENES[name]
        w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3))
        scene = gen()
        w.set_scene(scene)
        stream = torch.cuda.Stream()
        w.set_stream(stream.cuda_stream)   # the events below and the raycasts share one stream (not the null stream)
        torch.cuda.set_stream(stream)
        w.step_simulation(settle)
        aabb, _, _ = w.get_derived()
        shaped = scene["shape_type"] != scenes.SHAPE_PLANE
        lo, hi = aabb[shaped, :3].min(0), aabb[shaped, 3:].max(0)
        p0, p1 = rays(a.rays, lo - 2, hi + 2)
        t0 = torch.zeros((a.rays, 4), dtype=torch.float32, device=dev); t0[:, :3] = torch.from_numpy(p0).to(dev)
        t1 = torch.zeros((a.rays, 4), dtype=torch.float32, device=dev); t1[:, :3] = torch.from_numpy(p1).to(dev)
        out = torch.empty((a.rays, 8), dtype=torch.int32, device=dev)
        call = lambda n=a.rays: w.raycast_device(n, t0.data_ptr(), t1.data_ptr(), out.data_ptr())  # noqa: E731
        for _ in range(3):
            call()
        trace_ms = timed(call, a.reps)
        one_built = timed(lambda: call(1), a.reps)

        def rebuild_one():
            w.refresh_derived()   # a state change: the next raycast rebuilds boxes and tree
            call(1)
        refresh_only = timed(w.refresh_derived, a.reps)
        build_ms = timed(rebuild_one, a.reps) - refresh_only - one_built
        hits = out[:, 0].cpu().numpy().view(np.uint32)
        line = {"scene": name, "bodies": int(len(scene["kind"])), "rays": a.rays, "reps": a.reps,
                "raycast_ms": round(trace_ms, 4), "rays_per_s": round(a.rays / (trace_ms * 1e-3)),
                "tree_build_ms": round(build_ms, 4), "one_ray_call_ms": round(one_built, 4),
                "hit_fraction": round(float((hits != 0xFFFFFFFF).mean()), 4)}
        # (the reference's registry here holds at most 2^20 entities: the islands scene's bodies plus the manifolds of its first step
        # exceed it, so the baseline runs on the pile only)
        if a.cpu_rays and len(scene["kind"]) <= 65536 and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libedynref.so")):
            line["cpu_baseline"] = reference_baseline(w, scene, p0[:a.cpu_rays], p1[:a.cpu_rays], hits[:a.cpu_rays])
        print(json.dumps(line), flush=True)
        del w


if __name__ == "__main__":
    main()
