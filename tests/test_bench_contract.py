"""bench.py prints ONE JSON line with the driver's contract keys plus roofline / cpu_baseline objects (cpu_baseline and the other
legs beside the headline with --full)."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_json_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "pile512", "--steps", "10", "--warmup", "5",
                          "--cpu-sample-steps", "3", "--full"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 5 and d["higher_is_better"] is True
    assert d["unit"] == "steps/sec" and d["dtype"] == "f32" and d["vs_baseline"] is None and d["value"] > 0
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["finite"] is True
    assert d["config"]["settle_steps"] == 20 and d["config"]["colours"] >= 1 and "parity" in d["config"]
    # the headline is quoted on the reference's contact arithmetic; the opt-in forms are separate legs (default workload only)
    a = d["config"]["arithmetic"]
    assert a["mode"] == "reference" and list(a["steps_per_sec"]) == ["reference"] and abs(a["steps_per_sec"]["reference"] - d["value"]) < 1e-9
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    if r["traffic"] is None:   # no kept counter profile for this workload / schedule (pile512 has none): nothing is claimed
        assert r["achieved"] is None and r["frac"] is None and "no kept" in r["traffic_source"]
    else:
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["frac_from_algorithmic_bytes_only"] > 0 and r["algorithmic_bytes_per_launch"] > 0
    assert r["kernel"].startswith("k_contact_solve_df") and r["measured_read_ceiling"] > 1000 and r["measured_copy_ceiling"] > 1000
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    if c["kind"] == "reference":   # the real engine, multithreaded: both thread counts are in the sample text
        assert c["cores"] > 1 and "1-thread" in c["sample"] and "sequential_multithreaded" in c["sample"]


def test_bench_plain_run_is_the_headline_alone():
    """Without --full the line carries the headline, its config and the roofline of the timed steps - none of the legs that take
    runs of their own (other contact arithmetics, north_star, shim, CPU baseline, measured bandwidth ceilings). On the default workload,
    where --full runs every one of them."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "5"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["steps"] == 10 and d["warmup"] == 5 and d["value"] > 0 and abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-9 * d["ms_per_step"]
    assert d["unit"] == "steps/sec" and d["dtype"] == "f32" and d["higher_is_better"] is True and d["config"]["finite"] is True
    assert not {"cpu_baseline", "north_star", "shim"} & set(d)
    assert list(d["config"]["arithmetic"]["steps_per_sec"]) == ["reference"]
    r = d["roofline"]
    assert r["measured_read_ceiling"] is None and r["measured_copy_ceiling"] is None and r["frac_from_algorithmic_bytes_only"] > 0


def _two_rank_checks(out):
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0 and "cpu_baseline" not in d
    ns = d["north_star"]   # the sharded-islands leg: ONE scene over both ranks
    assert ns["n_gpus"] == 2 and ns["scaling"] == "strong" and ns["bodies"] == 64 * 64 + 1 and ns["bodies_this_rank"] == 32 * 64 + 1
    assert ns["steps_per_sec"] > 0 and ns["finite"] is True and isinstance(ns["meets_60hz"], bool)


def test_bench_two_ranks_on_one_gpu_functional():
    """The N>1 code path (rendezvous, per-step pack + all-gather, max-over-ranks timing, the sharded north_star leg) on a 1-GPU
    box: two ranks share cuda:0 and gather through gloo. The 8-GPU RCCL run itself is the driver's; this guards everything
    around it. Launched the way the driver launches it (torch.distributed.run) ..."""
    env = dict(os.environ, EDYN_BENCH_SHARE_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29600 + os.getpid() % 300), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "pile512",
           "--steps", "8", "--warmup", "4", "--north-star", "islands4k", "--north-star-steps", "6"]
    _two_rank_checks(subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env))


def test_bench_gpus_flag_starts_its_own_ranks():
    """... and as plain `python bench.py --gpus 2`: without torchrun's environment bench.py starts the two ranks itself
    (--gpus used to be parsed and ignored)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["EDYN_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "pile512", "--steps", "8", "--warmup", "4",
           "--north-star", "islands4k", "--north-star-steps", "6"]
    _two_rank_checks(subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env))


def test_bench_reports_every_contact_arithmetic_beside_the_headline():
    """the line carries steps/s of the headline workload in all three contact arithmetics - the default (the
    reference's operations) is `value`, the two opt-in forms are measured beside it with what each costs in parity."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "pile512", "--steps", "10", "--warmup", "5", "--north-star", "none",
                          "--other-arithmetic-steps", "10", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    a = d["config"]["arithmetic"]
    assert a["mode"] == "reference" and set(a["steps_per_sec"]) == {"reference", "fused_velocity_rows", "fused_rows_block_position"}
    assert all(v > 0 for v in a["steps_per_sec"].values()) and a["steps_per_sec"]["reference"] == d["value"]
    assert "NOT met" in a["other_modes"]["fused_rows_block_position"] and "zero error" in a["parity"]


def test_bench_four_ranks_on_one_gpu_functional():
    """the north_star leg with more ranks than two - 4 ranks, the islands sharded in contiguous site blocks, the
    per-step pack + all-gather of every rank's state - as a functional run on the one GPU of the test box (ranks share cuda:0, the gather goes
    through gloo). Four, not the eight of a node: a shared GPU is open in at most six processes at once, this test's own included (the
    launching bench.py leaves the device alone when ranks share it). The 8-GPU RCCL measurement itself is the driver's."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["EDYN_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--workload", "islands4k", "--steps", "6", "--warmup", "2",
           "--north-star", "islands4k", "--north-star-steps", "6"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and d["value"] > 0 and d["config"]["finite"] is True
    ns = d["north_star"]
    assert ns["n_gpus"] == 4 and ns["scaling"] == "strong" and ns["bodies"] == 64 * 64 + 1 and ns["bodies_this_rank"] == 16 * 64 + 1 and ns["finite"] is True


def test_bench_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """--dump-outputs DIR: the headline leg's last-step outputs (body state, contact manifolds) as float .npy files, within 64 MB;
    two runs with the same arguments write the same arrays, and ms_per_step is the time of one of the --steps timed steps."""
    dumps = []
    for run in ("a", "b"):
        d_out = tmp_path / run
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "pile512", "--steps", "7", "--warmup", "3",
                              "--north-star", "none", "--other-arithmetic-steps", "0", "--no-cpu-baseline", "--dump-outputs", str(d_out)],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
        assert d["steps"] == 7 and abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-9 * d["ms_per_step"]
        files = sorted(os.listdir(d_out))
        assert {"pos.npy", "orn.npy", "linvel.npy", "angvel.npy", "manifold_body.npy", "manifold_normal_impulse.npy"} <= set(files)
        assert sum(os.path.getsize(d_out / f) for f in files) <= 64 * 10 ** 6
        arrays = {f: np.load(d_out / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["pos.npy"].shape == (8 * 8 * 8 + 1, 3) and np.isfinite(arrays["pos.npy"]).all()
        assert len(arrays["manifold_body.npy"]) > 0
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
