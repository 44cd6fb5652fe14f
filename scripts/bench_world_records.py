"""What handing a multi-device world's result to the host costs: on pile32k (scenes.headline_pile(), 32 768 boxes on a plane) split into
2 shards, BOTH ON DEVICE 0, the wall time per hand-over, after a step, of

    get_state   edynhip_world_get_state into four caller arrays - the path the C++ shim took before the record hand-over existed: a host
                copy of what the step's gather already scattered (presentation, origins, flags and events are NOT part of it);
    records     edynhip_world_snapshot_records + edynhip_world_snapshot_map - every shard packs its bodies' 96-byte records and stores
                them into the world's pinned slot; the view is read in place (state, presentation, origin, flags, the event block).

    python scripts/bench_world_records.py [--rounds 5] [--reps 60] [--libs lanes1=edyn_amd/libedynhip.so,lanes6=/path/other.so] [--out profiles/world_records_bench.json]

The record kernel's lane mapping is a build-time choice (EDYNHIP_WORLD_RECORD_LANES of edyn_amd/csrc/world_records.hip: 1 = one lane per
record, the default; 6 = six lanes per record, one float4 each): --libs names one build per mapping (EDYNHIP_LIB selects it in a fresh child process)
and the rounds alternate between them. Every child builds the world, warms it up, then takes `reps` steps and times both hand-overs
after each (their order alternates from step to step); both calls are synchronous, so the wall clock around them is the cost. Per
variant the script reports the median over the rounds of the per-run medians and the spread (lowest and highest run median), prints one
JSON line and writes it to --out. A single pile is one island: one shard owns every box, the other reports nothing - the split costs the
second launch and event, not a second stream of stores. Stores from a second DEVICE into the shared slot are not measured here.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(reps, warm, shards):
    import numpy as np
    import edyn_amd
    from edyn_amd import _capi, scenes
    from edyn_amd.multi import MultiWorld
    L = _capi.lib()
    mw = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10, contact_events=True), devices=[0] * shards)
    mw.set_scene(scenes.headline_pile())
    mw.step_simulation(warm)
    n = mw.n
    pos = np.zeros((n, 3), np.float32); orn = np.zeros((n, 4), np.float32); lv = np.zeros((n, 3), np.float32); av = np.zeros((n, 3), np.float32)
    view = _capi.RecordView()
    ptr = [a.ctypes.data_as(C.c_void_p) for a in (pos, orn, lv, av)]

    def get_state():
        assert L.edynhip_world_get_state(mw._h, *ptr) == 0

    def records():
        assert L.edynhip_world_snapshot_records(mw._h, 0.004, 0xFFFFFFFF, 1) == 0
        assert L.edynhip_world_snapshot_map(mw._h, C.byref(view)) == 0

    for _ in range(4):
        mw.step_simulation(1); get_state(); records()
    took = {"get_state": [], "records": []}
    for k in range(reps):
        mw.step_simulation(1)
        for name, f in ((("get_state", get_state), ("records", records)) if k % 2 == 0 else (("records", records), ("get_state", get_state))):
            t = time.perf_counter(); f(); took[name].append((time.perf_counter() - t) * 1e6)
    # the two hand-overs agree on the state (the first 13 floats of a record)
    rec = np.ctypeslib.as_array((C.c_uint8 * (view.num_bodies * 96)).from_address(view.records)).view(_capi.RECORD_DTYPE)
    assert view.num_bodies == n and np.array_equal(rec["pos"], pos) and np.array_equal(rec["orn"], orn) and np.array_equal(rec["linvel"], lv) and np.array_equal(rec["angvel"], av)
    out = {"bodies": int(n), "bodies_per_shard": mw.get_stats()["bodies_per_shard"], "events_last_step": int(view.total_events),
           "get_state_us": round(statistics.median(took["get_state"]), 2), "records_us": round(statistics.median(took["records"]), 2)}
    mw.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--shards", type=int, default=2)
    ap.add_argument("--libs", default="lanes1=" + os.path.join(ROOT, "edyn_amd", "libedynhip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_records_bench.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.warm, a.shards)
        return
    libs = [tuple(x.split("=", 1)) for x in a.libs.split(",")]
    runs = {label: [] for label, _ in libs}
    for _ in range(a.rounds):          # alternating: one fresh process per build and round
        for label, path in libs:
            env = dict(os.environ, EDYNHIP_LIB=os.path.abspath(path))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warm", str(a.warm), "--shards", str(a.shards)],
                                 env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                raise SystemExit("child failed (%s): %s" % (label, out.stdout + out.stderr))
            runs[label].append(json.loads(line[0][7:]))

    def summary(values):
        return {"median_us": round(statistics.median(values), 2), "lowest_us": min(values), "highest_us": max(values), "runs_us": values}

    parent_path = [r["get_state_us"] for label, _ in libs for r in runs[label]]
    res = {"bench": "world_records", "scene": "pile32k", "shards": a.shards, "placement": "one GPU, every shard on device 0", "rounds": a.rounds, "reps_per_run": a.reps,
           "what": "wall microseconds per hand-over after a step: median over the runs of each run's median; get_state = the four-array copy (no presentation, origin, flags or events), records = snapshot_records + snapshot_map read in place",
           "bodies": runs[libs[0][0]][0]["bodies"], "bodies_per_shard": runs[libs[0][0]][0]["bodies_per_shard"],
           "get_state": summary(parent_path),
           "records": {label: summary([r["records_us"] for r in runs[label]]) for label, _ in libs}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
