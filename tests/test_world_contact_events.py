"""Contact events and point ids on a multi-device world (edynhip_world_get_contact_events / edynhip_world_get_point_ids,
MultiWorld.get_contact_events / .get_point_ids): 1, 2 and 3 shards on device 0 against ONE context holding the whole scene.

The contract: the application sees the single context's event stream - global body indices, the world's step count - and its point
identities; only the VALUES of the ids differ (a renaming that is a function, injective, and stable from POINT_CREATED to
POINT_DESTROYED), and a re-partition - by itself, forced, sticky or full - emits no event and changes no id.

The single context's side of every comparison is computed once per call pattern and shared by the shard counts."""
import ctypes as C
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd.multi import MultiWorld

pytestmark = pytest.mark.gpu
SHARDS = [1, 2, 3]
ERR_CAPACITY, ERR_UNSUPPORTED = -4, -6
CREATED, DESTROYED = _capi.EVENT_POINT_CREATED, _capi.EVENT_POINT_DESTROYED


def _bridge_scene():
    """tests/test_multirank_gloo.py::_bridge_scene(along="z"), re-stated: six mini-piles (six islands) plus a sphere that rolls from site 0
    into site 3, the row behind it - across the cut a world of 2 or 3 shards makes between the two rows of sites, which forces a
    re-partition with the contact manifolds carried along."""
    sc = scenes.mini_piles(3, 2)
    n = len(sc["kind"])
    ext = scenes._empty(n + 1)
    for k, v in sc.items():
        if k != "joints":
            ext[k][:n] = v
    ext["kind"][n] = scenes.KIND_DYNAMIC
    ext["pos"][n] = (-7.7, 0.5, -0.4)
    ext["linvel"][n] = (0, 0, 4.0)
    ext["shape_type"][n] = scenes.SHAPE_SPHERE; ext["shape_param"][n] = (0.5, 0, 0, 0)
    return ext


SCENES = {"bridge": _bridge_scene, "piles": lambda: scenes.mini_piles(2, 1)}
ONE_BY_ONE = (1,) * 90
MIXED_90 = tuple(1 + k % 3 for k in range(45))      # 1, 2, 3, 1, 2, 3, ...: 90 steps
MIXED_120 = tuple(1 + k % 3 for k in range(60))     # 120 steps
assert sum(MIXED_90) == 90 and sum(MIXED_120) == 120


def _cfg(**kw):
    return edyn_amd.init_config(num_solver_velocity_iterations=10, **kw)


def _single(scene, **kw):
    w = edyn_amd.World(_cfg(**kw)); w.set_scene(scene); scenes.apply_figure_settings(w, scene)
    return w


def _world(scene, shards, **kw):
    mw = MultiWorld(_cfg(**kw), devices=[0] * shards)
    mw.set_scene(scene)
    return mw


def _idless(ev):
    """The events without their ids as sorted rows (step, type, body[0], body[1])."""
    a = np.stack([ev["step"].astype(np.int64), ev["type"].astype(np.int64), ev["body"][:, 0].astype(np.int64), ev["body"][:, 1].astype(np.int64)], 1) \
        if len(ev) else np.zeros((0, 4), np.int64)
    return a[np.lexsort(a.T[::-1])]


def _with_ids(ev, kind, rename=None):
    """The point events of one kind as sorted rows (step, body[0], body[1], id); rename: world id -> single id."""
    e = ev[ev["type"] == kind]
    ids = [int(x) for x in e["point_id"]]
    if rename is not None:
        missing = [hex(x) for x in ids if x not in rename]
        assert not missing, ("event ids the id tables never showed", missing[:5])
        ids = [rename[x] for x in ids]
    return sorted(zip(e["step"].tolist(), e["body"][:, 0].tolist(), e["body"][:, 1].tolist(), ids))


class _Trace:
    pass


@functools.lru_cache(maxsize=None)
def _single_trace(scene_name, calls, sleeping=False):
    """One context through the call pattern: per call its events, manifold bodies and point ids; the final state."""
    w = _single(SCENES[scene_name](), contact_events=True, sleeping=sleeping)
    t = _Trace()
    t.calls = []
    for k in calls:
        w.step_simulation(k)
        t.calls.append((w.get_contact_events().copy(), w.get_manifolds()["body"].copy(), w.get_point_ids().copy(),
                        w.get_asleep().copy() if sleeping else None))
    t.state = [a.copy() for a in w.get_state()]
    return t


# ---- 1. equals one context, step by step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_equals_one_context_step_by_step(shards):
    ref = _single_trace("bridge", ONE_BY_ONE)
    mw = _world(_bridge_scene(), shards, contact_events=True)
    rename, back = {0: 0}, {0: 0}     # world id -> single id and the other way round, over the whole run
    born = {}                          # world id -> step of its POINT_CREATED
    first_repartition = None           # the call (= step) at whose end the first re-partition happened
    old_ids_destroyed_later = 0
    events_in_repartition_calls, seen_repartitions = [], 0
    for step, (es, bodies_s, ids_s, _) in enumerate(ref.calls):
        mw.step_simulation(1)
        ew = mw.get_contact_events()
        what = (shards, step)
        assert ew.dtype == es.dtype
        assert np.array_equal(_idless(ew), _idless(es)), what
        assert set(ew["step"].tolist()) <= {step}, what
        # destroyed points: the ids the dictionary knew BEFORE this call
        assert _with_ids(ew, DESTROYED, rename) == _with_ids(es, DESTROYED), what
        if first_repartition is not None:
            old_ids_destroyed_later += sum(1 for x in ew[ew["type"] == DESTROYED]["point_id"] if born[int(x)] <= first_repartition)
        # manifolds and the id tables, position by position
        assert np.array_equal(mw.get_manifolds()["body"], bodies_s), what
        ids_w = mw.get_point_ids()
        assert ids_w.dtype == ids_s.dtype and ids_w.shape == ids_s.shape, what
        assert np.array_equal(ids_w == 0, ids_s == 0), what
        for a, b in zip(ids_w.ravel().tolist(), ids_s.ravel().tolist()):
            assert rename.setdefault(a, b) == b, (what, hex(a), hex(b), hex(rename[a]))     # a function; a living id keeps its partner
            assert back.setdefault(b, a) == a, (what, hex(a), hex(b), hex(back[b]))         # injective
        # created points: mapped, the single context's ids per (step, body pair)
        assert _with_ids(ew, CREATED, rename) == _with_ids(es, CREATED), what
        for e in ew[ew["type"] == CREATED]:
            assert int(e["point_id"]) not in born, what
            born[int(e["point_id"])] = int(e["step"])
            assert int(e["point_id"]) >> 32 == int(e["step"]) + 1, what
        alive = ids_w[ids_w != 0]
        assert len(np.unique(alive)) == len(alive), what
        for x in alive.tolist():
            assert x in born and x >> 32 == born[x] + 1, (what, hex(x))
        reps = mw.get_stats()["repartitions"]
        if reps > seen_repartitions:
            seen_repartitions = reps
            if first_repartition is None:
                first_repartition = step
            events_in_repartition_calls.append((step, len(ew), len(es)))
    for got, want in zip(mw.get_state(), ref.state):
        assert np.array_equal(got, want)
    if shards >= 2:
        assert mw.get_stats()["repartitions"] >= 1
        assert old_ids_destroyed_later >= 1, "no point created before the first re-partition was destroyed after it"
        for step, n_world, n_single in events_in_repartition_calls:   # (equal as multisets above: none extra, none missing)
            assert n_world == n_single, step
    mw.close()


# ---- 2. multi-step calls -------------------------------------------------------------------------------------------------------------
def _world_asleep(mw):
    """The sleeping flags of the whole world from the shards' contexts (read-only use): a shard holds, in ascending global order, the
    bodies it owns and a replica of every non-dynamic one; every body's flag is taken from the shard that owns it (shard 0: the replicas)."""
    L = _capi.lib()
    part = mw.get_partition()
    out = np.zeros(mw.n, np.uint8)
    for r in range(mw.num_shards):
        ctx = L.edynhip_world_context(mw._h, r)
        members = np.flatnonzero((part == r) | (part < 0))
        if not ctx or len(members) == 0:
            continue
        local = np.zeros(len(members), np.uint8)
        assert L.edynhip_get_asleep(C.c_void_p(ctx), local.ctypes.data) == 0
        mine = (part[members] == r) | ((part[members] < 0) & (r == 0))
        out[members[mine]] = local[mine]
    return out


def _compare_calls(mw, ref, calls, what):
    done = 0
    for call, k in enumerate(calls):
        mw.step_simulation(k)
        ew, es, asleep = mw.get_contact_events(), ref.calls[call][0], ref.calls[call][3]
        assert np.array_equal(_idless(ew), _idless(es)), (what, call)
        assert all(done <= s < done + k for s in ew["step"].tolist()), (what, call)
        if asleep is not None:
            assert np.array_equal(_world_asleep(mw), np.asarray(asleep, np.uint8)), (what, call)
        done += k
    for got, want in zip(mw.get_state(), ref.state):
        assert np.array_equal(got, want), what


@pytest.mark.parametrize("shards", SHARDS)
def test_multi_step_calls(shards):
    mw = _world(_bridge_scene(), shards, contact_events=True)
    _compare_calls(mw, _single_trace("bridge", MIXED_90), MIXED_90, shards)
    if shards >= 2:
        assert mw.get_stats()["repartitions"] >= 1
    mw.close()


# ---- 3. forced re-partition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_forced_repartition_emits_nothing_and_keeps_every_id(shards):
    calls = (10, 1)
    ref = _single_trace("piles", calls)
    mw = _world(scenes.mini_piles(2, 1), shards, contact_events=True)
    mw.step_simulation(10)
    events, ids = mw.get_contact_events(), mw.get_point_ids()
    assert np.array_equal(_idless(events), _idless(ref.calls[0][0]))
    assert (ids != 0).sum() > 100
    before = mw.get_stats()["repartitions"]
    mw.repartition()
    assert mw.get_stats()["repartitions"] == before + 1
    assert np.array_equal(mw.get_contact_events(), events)     # still the events of the last step call, record for record
    assert np.array_equal(mw.get_point_ids(), ids)             # element for element
    rename = dict(zip(ids.ravel().tolist(), ref.calls[0][2].ravel().tolist()))
    assert rename.get(0, 0) == 0
    mw.step_simulation(1)
    ew, (es, bodies_s, ids_s, _) = mw.get_contact_events(), ref.calls[1]
    assert np.array_equal(_idless(ew), _idless(es))
    assert _with_ids(ew, DESTROYED, rename) == _with_ids(es, DESTROYED)
    assert np.array_equal(mw.get_manifolds()["body"], bodies_s)
    ids_w = mw.get_point_ids()
    assert ids_w.shape == ids_s.shape
    for a, b in zip(ids_w.ravel().tolist(), ids_s.ravel().tolist()):
        assert rename.setdefault(a, b) == b, (hex(a), hex(b))
    assert len(set(rename.values())) == len(rename)
    mw.close()


# ---- 4. sleeping on ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_sleeping_on(shards):
    mw = _world(_bridge_scene(), shards, contact_events=True, sleeping=True)
    _compare_calls(mw, _single_trace("bridge", MIXED_120, True), MIXED_120, shards)
    mw.close()


# ---- 5. flag off ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_flag_off_is_unsupported_and_steps_the_same(shards):
    off = _world(_bridge_scene(), shards)
    on = _world(_bridge_scene(), shards, contact_events=True)
    single = _single(_bridge_scene())
    for w in (off, on, single):
        w.step_simulation(30)
    for f in (off.get_contact_events, off.get_point_ids):
        with pytest.raises(edyn_amd.EdynHipError) as ei:
            f()
        assert ei.value.code == ERR_UNSUPPORTED
    for a, b, c in zip(off.get_state(), on.get_state(), single.get_state()):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    off.close(); on.close()


# ---- 6. arguments --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_arguments(shards):
    L = _capi.lib()
    mw = _world(scenes.mini_piles(2, 1), shards, contact_events=True)
    n, m = C.c_uint32(99), C.c_uint32(99)
    # described, not stepped: no events, no manifolds
    assert L.edynhip_world_get_contact_events(mw._h, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.edynhip_world_get_point_ids(mw._h, None, 0, C.byref(m)) == 0 and m.value == 0
    assert len(mw.get_contact_events()) == 0 and mw.get_point_ids().shape == (0, 4) and len(mw.get_manifolds()) == 0
    mw.step_simulation(3)
    assert L.edynhip_world_get_contact_events(mw._h, None, 0, C.byref(n)) == 0 and n.value > 100     # out == NULL: the count
    assert L.edynhip_world_get_point_ids(mw._h, None, 0, C.byref(m)) == 0 and m.value == len(mw.get_manifolds()) > 0
    out = np.zeros(n.value, _capi.EVENT_DTYPE)
    k = C.c_uint32(0)
    assert L.edynhip_world_get_contact_events(mw._h, out.ctypes.data, n.value - 1, C.byref(k)) == ERR_CAPACITY and k.value == n.value
    assert not out.view(np.uint8).any()                                                              # nothing was written
    assert L.edynhip_world_get_contact_events(mw._h, out.ctypes.data, n.value, C.byref(k)) == 0 and k.value == n.value
    assert np.array_equal(out, mw.get_contact_events())
    ids = np.zeros((m.value, 4), np.uint64)
    assert L.edynhip_world_get_point_ids(mw._h, ids.ctypes.data, m.value - 1, C.byref(k)) == ERR_CAPACITY and k.value == m.value
    assert L.edynhip_world_get_point_ids(mw._h, ids.ctypes.data, m.value, C.byref(k)) == 0 and np.array_equal(ids, mw.get_point_ids())
    mw.close()
