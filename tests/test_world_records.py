"""Record hand-over of a multi-device world (edynhip_world_snapshot_records / edynhip_world_snapshot_map, MultiWorld.snapshot_records /
.snapshot_map): 1, 2, 3 and 5 shards on device 0 against ONE context holding the whole scene (World.snapshot_records / .snapshot_map -
existing code, not the code under test).

The contract: after every step call the world's records equal the single context's byte for byte - state, presentation at present_dt,
origin and flags, by global body index - with the same step_index; the view's event block is the head of get_contact_events(), its total
the number of events that occurred; a view stays valid until the next-but-one snapshot.

The scene (37 bodies): a plane, four separated box piles of 16, 8, 4 and 4 boxes along z (unequal, so that the cut between pile 0 and
pile 1 exists for 2, 3 and 5 shards), a sphere that rolls from pile 0 into pile 1 (a re-partition mid-run), two boxes of pile 1 with
centre-of-mass offsets, a moving kinematic box, a sphere spinning at 25 rad/s and a box with |w| = 0.0005 (both branches of integrate).
Five shards are more than there are heavy islands: shard 0 is left with the replicated bodies only.

The single context's side of every comparison is computed once per scenario and shared by the shard counts."""
import ctypes as C
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd.multi import MultiWorld

pytestmark = pytest.mark.gpu
SHARDS = [1, 2, 3, 5]
ERR_INVALID = -1
CALLS = (1, 1, 3, 1) * 20                                   # 120 steps
PRESENT = tuple(0.004 if k % 2 else 0.0 for k in range(len(CALLS)))
assert sum(CALLS) == 120
PILES = ((4, 2, 2), (2, 2, 2), (2, 1, 2), (2, 1, 2))        # nx, ny, nz: 16, 8, 4, 4 boxes
PILE_Z = (-12.0, -4.0, 4.0, 12.0)
SPHERE, KINEMATIC, FAST, SLOW, N = 33, 34, 35, 36, 37
REC = _capi.RECORD_DTYPE


def _scene():
    s = scenes._empty(N)
    scenes._add_plane(s)
    at = 1
    for (nx, ny, nz), z in zip(PILES, PILE_Z):
        pos, _ = scenes._lattice(nx, ny, nz, origin=(0.0, 0.0, z))
        s["pos"][at:at + len(pos)] = pos
        at += len(pos)
    assert at == SPHERE
    s["shape_type"][1:SPHERE] = scenes.SHAPE_BOX
    s["shape_param"][1:SPHERE, :3] = 0.5
    scenes._jitter(s, 1, SPHERE - 1)
    s["kind"][1:] = scenes.KIND_DYNAMIC
    s["pos"][SPHERE] = (0.2, 0.5, -9.3); s["linvel"][SPHERE] = (0, 0, 6.0)
    s["shape_type"][SPHERE] = scenes.SHAPE_SPHERE; s["shape_param"][SPHERE] = (0.5, 0, 0, 0)
    s["kind"][KINEMATIC] = scenes.KIND_KINEMATIC
    s["pos"][KINEMATIC] = (6.0, 3.0, 0.0); s["linvel"][KINEMATIC] = (0.5, 0, 0); s["angvel"][KINEMATIC] = (0, 0.3, 0)
    s["shape_type"][KINEMATIC] = scenes.SHAPE_BOX; s["shape_param"][KINEMATIC, :3] = 0.25
    s["pos"][FAST] = (-5.0, 0.5, 8.0); s["angvel"][FAST] = (0, 25.0, 0)
    s["shape_type"][FAST] = scenes.SHAPE_SPHERE; s["shape_param"][FAST] = (0.5, 0, 0, 0)
    s["pos"][SLOW] = (5.0, 0.5, 8.0); s["angvel"][SLOW] = (0, 0.0005, 0)
    s["shape_type"][SLOW] = scenes.SHAPE_BOX; s["shape_param"][SLOW, :3] = 0.5
    com = np.zeros((N, 3), np.float32)
    com[18] = (0.1, 0.0, 0.05); com[21] = (0.0, 0.1, 0.0)      # two boxes of pile 1 (bodies 17 .. 24)
    s["com"] = com
    return s


def _two_boxes():
    s = scenes._empty(2)
    s["kind"][:] = scenes.KIND_DYNAMIC
    s["pos"][0] = (0.3, 3.2, -4.0); s["pos"][1] = (-6.0, 0.5, -8.0)      # one drops onto pile 1, one lands on the plane by itself
    s["shape_type"][:] = scenes.SHAPE_BOX; s["shape_param"][:, :3] = 0.5
    return s


def _cfg(**kw):
    return edyn_amd.init_config(num_solver_velocity_iterations=10, **kw)


def _single(room=0, **kw):
    sc = _scene()
    w = edyn_amd.World(_cfg(max_bodies=N + room, **kw)); w.set_scene(sc); scenes.apply_figure_settings(w, sc)
    return w


def _world(shards, **kw):
    mw = MultiWorld(_cfg(**kw), devices=[0] * shards)
    mw.set_scene(_scene())
    return mw


def _idless(ev):
    """The events without their ids as sorted rows (step, type, body[0], body[1])."""
    a = np.stack([ev["step"].astype(np.int64), ev["type"].astype(np.int64), ev["body"][:, 0].astype(np.int64), ev["body"][:, 1].astype(np.int64)], 1) \
        if len(ev) else np.zeros((0, 4), np.int64)
    return a[np.lexsort(a.T[::-1])]


def _snap(w, present_dt=0.0, max_events=1 << 20):
    w.snapshot_records(present_dt, max_events)
    return w.snapshot_map()


def _same_records(got, want, what):
    assert got.dtype == want.dtype == REC and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError((what, "bodies that differ", bad[:8], got[bad[0]], want[bad[0]]))


def _check_handover(mw, want, present_dt, what):
    """One hand-over of the world against the single context's (records, events, total, step): records and step_index equal; the event
    block = the head of get_contact_events(), record for record; id-less and sorted, the single context's events."""
    rec_s, ev_s, total_s, step_s = want
    rec, ev, total, step = _snap(mw, present_dt)
    _same_records(rec, rec_s, what)
    assert step == step_s, what
    if ev_s is None:
        return
    listed = mw.get_contact_events()
    assert total == len(listed) == total_s, what
    assert len(ev) == len(listed) and ev.tobytes() == listed.tobytes(), what
    assert np.array_equal(_idless(ev), _idless(ev_s)), what


# ---- the single context's side, once per scenario ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run_trace(events):
    w = _single(contact_events=events)
    out = []
    for k, dt in zip(CALLS, PRESENT):
        w.step_simulation(k)
        rec, ev, total, step = _snap(w, dt)
        out.append((rec, ev if events else None, total, step))
    return out


@functools.lru_cache(maxsize=None)
def _sleep_trace():
    w = _single(contact_events=True, sleeping=True)
    out = []
    while len(out) < 40:                       # 10 steps per call, at most 400 steps
        w.step_simulation(10)
        out.append(_snap(w, 0.004))
        asleep = (out[-1][0]["flags"] & _capi.RECORD_ASLEEP) != 0
        if asleep[1:SPHERE].any() and len(out) % 2 == 0:
            break
    return out


# ---- 1. the run: every call equals one context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_records_equal_one_context_after_every_call(shards):
    ref = _run_trace(True)
    assert any(((r[0]["angvel"] ** 2).sum(1) > 1.0).any() for r in ref) and all(((r[0]["flags"] & _capi.RECORD_HAS_ORIGIN) != 0).sum() == 2 for r in ref)
    mw = _world(shards, contact_events=True)
    reps_at = []
    for call, (k, dt) in enumerate(zip(CALLS, PRESENT)):
        mw.step_simulation(k)
        _check_handover(mw, ref[call], dt, (shards, call))
        reps_at.append(mw.get_stats()["repartitions"])
    if shards >= 2:   # the sphere left pile 0's shard for pile 1's: the run went through a re-partition, and not only at its very end
        assert reps_at[-1] >= 1 and reps_at[len(reps_at) // 8] == 0 and reps_at[-8] >= 1, reps_at
    if shards == 5:   # one shard never owned a body, and shard 0 - the sphere gone to pile 1's shard - reports the replicated bodies only
        per_shard = mw.get_stats()["bodies_per_shard"]
        assert min(per_shard) == 0 and per_shard[0] == 2, per_shard
    mw.close()


@pytest.mark.parametrize("shards", [2, 5])
def test_world_without_the_events_flag(shards):
    ref = _run_trace(False)
    mw = _world(shards)
    for call in range(12):
        mw.step_simulation(CALLS[call])
        mw.snapshot_records(PRESENT[call], 4096)
        v = mw.snapshot_view()
        assert not v.events and v.num_events == 0 and v.total_events == 0
        rec, ev, total, step = mw.snapshot_map()
        _same_records(rec, ref[call][0], (shards, call))
        assert len(ev) == 0 and total == 0 and step == ref[call][3]
    mw.close()


# ---- 2. events -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 3])
def test_event_block_is_cut_at_max_events(shards):
    mw = _world(shards, contact_events=True)
    mw.step_simulation(1)
    listed = mw.get_contact_events()
    assert len(listed) > 2                       # the first step creates every manifold of the piles
    rec, ev, total, step = _snap(mw, 0.0, max_events=2)
    assert len(ev) == 2 < total == len(listed) and ev.tobytes() == listed[:2].tobytes()
    rec, ev, total, step = _snap(mw, 0.0, max_events=0)
    assert len(ev) == 0 and total == len(listed)
    rec, ev, total, step = _snap(mw, 0.0)
    assert ev.tobytes() == listed.tobytes() and total == len(listed) and step == 1
    mw.close()


# ---- 3. sleeping, edits, a forced re-partition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [3])
def test_sleeping_bit(shards):
    ref = _sleep_trace()
    assert ((ref[-1][0]["flags"][1:SPHERE] & _capi.RECORD_ASLEEP) != 0).any(), "no pile fell asleep in 400 steps"
    mw = _world(shards, contact_events=True, sleeping=True)
    for call, want in enumerate(ref):
        mw.step_simulation(10)
        _check_handover(mw, want, 0.004, (shards, call))
    mw.close()


@pytest.mark.parametrize("shards", [2, 5])
def test_edits_and_forced_repartition(shards):
    w, mw = _single(room=8, contact_events=True), _world(shards, contact_events=True)

    def both(what, dt=0.004, events=True):
        want = _snap(w, dt)
        _check_handover(mw, want if events else (want[0], None, 0, want[3]), dt, (shards, what))
        return want[0]

    for x in (w, mw):
        x.step_simulation(20)
    both("settled")
    # remove_bodies: a box of pile 0 - the tombstone before and after the step that drops it, and after every shard was rebuilt
    for x in (w, mw):
        x.remove_bodies([5])
    rec = both("removed, not stepped", events=False)
    assert rec["flags"][5] & _capi.RECORD_REMOVED and not (rec["flags"][5] & _capi.RECORD_DYNAMIC)
    for x in (w, mw):
        x.step_simulation(1)
    assert both("removed, stepped")["flags"][5] & _capi.RECORD_REMOVED
    before = mw.get_stats()["repartitions"]
    first = _snap(mw, 0.004)
    mw.repartition()                                            # between two snapshots: nothing the application sees may change
    assert mw.get_stats()["repartitions"] == before + 1
    second = _snap(mw, 0.004)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2:] == second[2:]
    assert both("re-partitioned")["flags"][5] & _capi.RECORD_REMOVED
    for x in (w, mw):
        x.step_simulation(3)
    both("re-partitioned, stepped")
    # add_scene: two boxes - num_bodies grows past what the slots were first sized for
    assert w.add_scene(_two_boxes()) == N and mw.add_scene(_two_boxes())[0] == N
    rec = both("added, not stepped", events=False)
    assert len(rec) == N + 2
    for x in (w, mw):
        x.step_simulation(2)
    assert len(both("added, stepped")) == N + 2
    for x in (w, mw):
        x.step_simulation(1)
    both("added, the other slot")
    # set_state: lift a box of pile 2 and throw the fast sphere
    pos, orn, lv, av = [a.copy() for a in w.get_state()]
    pos[26] += (0, 1.5, 0); lv[FAST] = (1.0, 2.0, 0.0); av[FAST] = (3.0, 0.0, 0.0)
    for x in (w, mw):
        x.set_state(pos, orn, lv, av)
    both("state set, not stepped", events=False)
    for k in (1, 4):
        for x in (w, mw):
            x.step_simulation(k)
        both(("state set, stepped", k))
    mw.close()


# ---- 4. slot lifetime, arguments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2])
def test_a_view_stays_valid_until_the_next_but_one_snapshot(shards):
    mw = _world(shards, contact_events=True)
    mw.step_simulation(1)
    mw.snapshot_records(0.004, 4096)
    a = mw.snapshot_view()
    assert a.num_bodies == N and a.num_events > 0 and a.step_index == 1
    rec_a = C.string_at(a.records, a.num_bodies * REC.itemsize)
    ev_a = C.string_at(a.events, a.num_events * _capi.EVENT_DTYPE.itemsize)
    mw.step_simulation(2)
    mw.snapshot_records(0.0, 4096)
    b = mw.snapshot_view()
    assert b.records != a.records and b.step_index == 3
    rec_b = C.string_at(b.records, b.num_bodies * REC.itemsize)
    assert rec_b != rec_a                                                         # the world moved on ...
    assert C.string_at(a.records, a.num_bodies * REC.itemsize) == rec_a          # ... and view A still shows step 1
    assert C.string_at(a.events, a.num_events * _capi.EVENT_DTYPE.itemsize) == ev_a
    mw.step_simulation(1)
    mw.snapshot_records(0.0, 4096)                                                # (A's slot may be overwritten from here on)
    c = mw.snapshot_view()
    assert c.step_index == 4 and C.string_at(b.records, b.num_bodies * REC.itemsize) == rec_b
    mw.close()


def _state_after_five_steps():
    mw = _world(2)
    mw.step_simulation(5)
    state = b"".join(np.ascontiguousarray(a).tobytes() for a in mw.get_state())
    mw.close()
    return state


def test_destroy_before_the_build_and_with_a_pack_pending():
    """The two ways out of a world that no other test takes: destroyed as described, before any shard exists, and destroyed right behind a
    snapshot nobody mapped, while the shards' packs into the pinned slot may still be running. Both return quietly and leave the device as
    a process that never did either finds it: a world made afterwards steps to the state a fresh process computes (this file run as a
    script)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    fresh = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert fresh.returncode == 0, fresh.stderr[-2000:]
    mw = _world(2, contact_events=True)
    mw.close()                                                                    # described, never built
    mw = _world(2, contact_events=True)
    mw.step_simulation(5)
    mw.snapshot_records(0.004, 4096)
    mw.close()                                                                    # both shards' packs and the event block are out
    assert _state_after_five_steps().hex() == fresh.stdout.strip()


def test_arguments():
    L = _capi.lib()
    mw = _world(2, contact_events=True)
    v = _capi.RecordView()
    assert L.edynhip_world_snapshot_map(mw._h, C.byref(v)) == ERR_INVALID       # no snapshot yet
    assert "no record snapshot" in L.edynhip_world_last_error(mw._h).decode()
    for flags in (2, 3, 0x80000000):
        assert L.edynhip_world_snapshot_records(mw._h, 0.0, 16, flags) == ERR_INVALID
    assert L.edynhip_world_snapshot_map(mw._h, None) == ERR_INVALID
    # described, not stepped: the described state, step 0, no events; EDYNHIP_SNAPSHOT_DIRECT is accepted
    assert L.edynhip_world_snapshot_records(mw._h, 0.0, 16, _capi_direct()) == 0
    rec, ev, total, step = mw.snapshot_map()
    w = _single(contact_events=True)
    _same_records(rec, _snap(w)[0], "described")
    assert len(ev) == 0 and total == 0 and step == 0
    mw.close()


def _capi_direct():
    return 1   # EDYNHIP_SNAPSHOT_DIRECT


if __name__ == "__main__":   # the fresh process of test_destroy_before_the_build_and_with_a_pack_pending
    print(_state_after_five_steps().hex())
