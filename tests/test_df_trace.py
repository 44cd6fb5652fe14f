"""The trace stamps of the dataflow kernels (EDYNHIP_DF_TRACE / EDYNHIP_DFP_TRACE with EDYNHIP_DF_TRACE_STEP): four wall-clock stamps
per (sweep, round, wave), written by each kernel's hand-off loop on its way out. The knobs change nothing a step computes (tests/test_knobs.py
lists them as output-only), so no parity test sees them; this file holds the stamps to what the loop promises.

File, as launch_velocity / launch_position write it: {na, stride, sweeps, per_wave} as uint32, na sorted colour keys (uint32), then
sweeps x rounds x waves records of four uint64, rounds = ceil(na / stride), waves = stride / per_wave ("sweeps" = position iterations in
a position trace). A record is (w0 task begins, w1 first look at the own slots is back, w2 the inputs of the wave's colour are in,
w3 the task is finished). The wave of a record had a task when round * stride + wave * per_wave < na; every other record stays zero.

w1 stays 0 where no lane had to poll (the one-lane kernel stamps it with its first poll). w2 stays 0 where no lane of the wave ever had a
turn: in a position iteration after the first, the lanes of an island that met the error threshold are finished before they begin
(island_solver.cpp:350-353), and a wave of such lanes leaves in its first round. Measured on the scene below: 16 waves x 3 iterations,
w2 == 0 in 32 of the 48 records.
So w2 == 0 is accepted in position iterations >= 1 only; every velocity record and every record of the first position iteration must
carry w0 <= w2 <= w3."""
import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes

pytestmark = pytest.mark.gpu

CASES = [("EDYNHIP_DF_TRACE", 1), ("EDYNHIP_DF_TRACE", 2), ("EDYNHIP_DF_TRACE", 4), ("EDYNHIP_DFP_TRACE", None)]


@pytest.mark.parametrize("knob,lanes", CASES, ids=["velocity_lanes1", "velocity_lanes2", "velocity_lanes4", "position"])
def test_trace_stamps_are_ordered_and_only_waves_with_a_task_write_them(monkeypatch, tmp_path, knob, lanes):
    path = tmp_path / "trace.bin"
    monkeypatch.setenv(knob, str(path))
    monkeypatch.setenv("EDYNHIP_DF_TRACE_STEP", "5")
    if lanes is not None:
        monkeypatch.setenv("EDYNHIP_DF_LANES", str(lanes))
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3))
    w.set_scene(scenes.box_pile(6, 6, 6, mixed=True))
    for name in (knob, "EDYNHIP_DF_TRACE_STEP", "EDYNHIP_DF_LANES"):   # (the library reads them when the context is created)
        monkeypatch.delenv(name, raising=False)
    w.step_simulation(10)

    raw = path.read_bytes()
    na, stride, sweeps, per_wave = (int(x) for x in np.frombuffer(raw[:16], np.uint32))
    assert per_wave == (32 if lanes is None else 64 // lanes)   # the kernel the case names ran: a four-lane request can fall back to two lanes
    assert na > 0 and stride % per_wave == 0
    assert sweeps == (3 if lanes is None else 11)
    rounds, waves = (na + stride - 1) // stride, stride // per_wave
    assert len(raw) == 16 + 4 * na + 8 * 4 * sweeps * rounds * waves   # the size that follows from the file's own header
    tr = np.frombuffer(raw[16 + 4 * na:], np.uint64).reshape(sweeps, rounds, waves, 4)
    r, v = np.meshgrid(np.arange(rounds), np.arange(waves), indexing="ij")
    task = np.broadcast_to(r * stride + v * per_wave < na, (sweeps, rounds, waves))
    print("na %d stride %d sweeps %d per_wave %d: %d records with a task, %d without; w1 == 0 in %d, w2 == 0 in %d" %
          (na, stride, sweeps, per_wave, task.sum(), (~task).sum(), (tr[task][:, 1] == 0).sum(), (tr[task][:, 2] == 0).sum()))
    assert task.any()
    w0, w1, w2, w3 = (tr[task][:, k] for k in range(4))
    assert (w0 > 0).all()
    assert (w0 <= w3).all()
    no_turn = np.broadcast_to(np.arange(sweeps)[:, None, None] >= (1 if lanes is None else sweeps), task.shape)[task] & (w2 == 0)
    assert ((w0 <= w2) & (w2 <= w3))[~no_turn].all()
    assert ((w1 == 0) | ((w0 <= w1) & (w1 <= w3))).all()
    assert not tr[~task].any()
