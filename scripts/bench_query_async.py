"""The ticketed queries, measured (DESIGN §8 "Queries in asynchronous mode"). Prints one JSON line; --out writes it to a file too.

    python scripts/bench_query_async.py [--parts submit,interest] [--reps R] [--out FILE]

submit    on the settled headline pile, with 8 steps enqueued just before: the host time of edynhip_raycast_submit for 1, 64 and 4096
          rays, of edynhip_raycast for the same rays, and the time the enqueued steps still take (a synchronise after); and the same
          submit with nothing in flight. A submit that does not wait stays below the synchronous call and does not grow with the work
          in flight.
interest  on the 262 144-box islands scene: a ticket of 1 and of 1024 boxes (a pile's size) that want the of-interest list, submit to
          collect, against the same boxes wanting the islands list only - the difference is the marked pass over the bodies, whose
          model is 2 passes x boxes x ceil(bodies / 64) wave iterations.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import edyn_amd  # noqa: E402
from edyn_amd import _capi, scenes  # noqa: E402


def world(scene, steps):
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3))
    w.set_scene(scene)
    w.step_simulation(steps)
    w.synchronize()
    return w


def us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def part_submit(reps):
    w = world(scenes.headline_pile(), 300)
    L, h = w._L, w._h
    pos = w.get_state()[0]
    lo, hi = pos.min(0), pos.max(0)
    rng = np.random.default_rng(3)
    out = {"scene": "pile32k", "bodies": int(w.n), "steps_in_flight": 8, "rays": {}}
    for n in (1, 64, 4096):
        a = np.ascontiguousarray(np.stack([rng.uniform(lo[0], hi[0], n), np.full(n, hi[1] + 5), rng.uniform(lo[2], hi[2], n)], 1).astype(np.float32))
        b = np.ascontiguousarray((a * np.float32([1, 0, 1]) + np.float32([0.3, -1, -0.2])).astype(np.float32))
        hits = np.zeros(n, _capi.RAYCAST_HIT_DTYPE)
        t = C.c_uint64(0)
        pa, pb, ph = a.ctypes.data, b.ctypes.data, hits.ctypes.data

        def submit():
            assert L.edynhip_raycast_submit(h, n, pa, pb, None, None, 0, C.byref(t)) == 0

        def release():
            p, m = C.c_void_p(None), C.c_uint32(0)
            assert L.edynhip_raycast_collect(h, t.value, C.byref(p), C.byref(m)) == 0 and L.edynhip_query_release(h, t.value) == 0

        submit(); release()   # buffers
        assert L.edynhip_raycast(h, n, pa, pb, 0, None, 0, ph) == 0
        rows = {"submit_us": [], "tail_after_submit_us": [], "submit_idle_us": [], "submit_one_step_us": [], "sync_call_us": [], "step_call_us": [], "collect_us": []}
        for _ in range(reps):
            rows["step_call_us"].append(us(lambda: L.edynhip_step(h, 8)))
            rows["submit_us"].append(us(submit))
            rows["tail_after_submit_us"].append(us(lambda: L.edynhip_synchronize(h)))
            rows["collect_us"].append(us(release))
            rows["submit_idle_us"].append(us(submit))   # nothing in flight, the query tree still current
            release()
            L.edynhip_step(h, 1)
            rows["submit_one_step_us"].append(us(submit))   # one step in flight instead of eight: the tree is rebuilt all the same
            release()
            L.edynhip_step(h, 8)
            rows["sync_call_us"].append(us(lambda: L.edynhip_raycast(h, n, pa, pb, 0, None, 0, ph)))
            L.edynhip_synchronize(h)
        out["rays"][str(n)] = {k: round(statistics.median(v), 2) for k, v in rows.items()}
    w.detach()
    return out


def part_interest(reps):
    scene = scenes.c4_islands()
    w = world(scene, 120)
    pos = w.get_state()[0]
    rng = np.random.default_rng(4)
    out = {"scene": "islands256k", "bodies": int(w.n), "boxes": {}}
    for n in (1, 1024):
        c = pos[rng.integers(1, w.n, n)]
        q = np.concatenate([c - 2.5, c + 2.5], axis=1).astype(np.float32)
        res = {}
        for name, want in (("islands_only", _capi.WANT_ISLANDS), ("of_interest", _capi.WANT_ISLANDS | _capi.WANT_OF_INTEREST)):
            probe = w.query_aabb_submit(q, want, 0)
            try:
                w.query_collect(probe)
                total = 0
            except edyn_amd.EdynHipError as e:
                total = e.total
            w.query_release(probe)
            times = []
            for _ in range(reps):
                w.synchronize()
                t0 = time.perf_counter()
                t = w.query_aabb_submit(q, want, total)
                off, ids = w.query_collect(t)
                times.append((time.perf_counter() - t0) * 1e3)
                w.query_release(t)
            res[name] = {"ms": round(statistics.median(times), 4), "ids": int(total)}
        res["marked_pass_ms"] = round(res["of_interest"]["ms"] - res["islands_only"]["ms"], 4)
        res["model_wave_iterations"] = 2 * n * ((w.n + 63) // 64)
        res["ns_per_wave_iteration"] = round(1e6 * res["marked_pass_ms"] / res["model_wave_iterations"], 3)
        out["boxes"][str(n)] = res
    w.detach()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="submit,interest")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {}
    for p in a.parts.split(","):
        res[p] = {"submit": part_submit, "interest": part_interest}[p](a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
