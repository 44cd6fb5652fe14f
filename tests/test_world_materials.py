"""Materials on a multi-device world (edynhip_world_set_material_extras / _set_material_ids / _insert_material_mixing /
_get_point_extras; MultiWorld.set_material_extras ...): 1, 2 and 3 shards on device 0 against ONE context holding the whole scene,
whose materials tests/test_gpu_parity.py::test_contact_extras_bit_exact holds to the oracle.

The contract: bit for bit the single context's state, manifolds, point extras and - with events on - event stream and point identities
after every call, through re-partitions: a contact point keeps the material it was created with and the warm-start impulses of its
rolling pair and spinning row wherever its island goes.

The single context's side of a comparison is computed once and shared by the shard counts."""
import ctypes as C
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd.multi import MultiWorld

pytestmark = pytest.mark.gpu
SHARDS = [1, 2, 3]
ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -4, -6
LARGE = np.float32(1e18)
MIXED_120 = tuple(1 + k % 3 for k in range(60))     # 1, 2, 3, 1, 2, 3, ...: 120 steps
MIXED_90 = tuple(1 + k % 3 for k in range(45))
assert sum(MIXED_120) == 120 and sum(MIXED_90) == 90
SPHERE, CAPSULE, CYLINDER = 385, 386, 387           # _bridge_scene: the three rollers behind the plane and the 6 x 64 boxes
SOFT = slice(1, 1 + 64)                             # the pile of site 0, beside which the rollers start
STIFF, DAMP = 3000.0, 30.0                          # soft contacts a resting pile of unit boxes stays a pile with


def _bridge_scene():
    """tests/test_world_contact_events.py::_bridge_scene, re-stated: six mini-piles (six islands) plus a sphere that rolls from site 0 into
    site 3, the row behind it - across the cut a world of 2 or 3 shards makes between the two rows of sites, which forces a re-partition
    with the contact manifolds carried along. Beside the sphere a capsule and a cylinder on their sides roll the same way."""
    sc = scenes.mini_piles(3, 2)
    n = len(sc["kind"])
    ext = scenes._empty(n + 3)
    for k, v in sc.items():
        if k != "joints":
            ext[k][:n] = v
    ext["kind"][n:] = scenes.KIND_DYNAMIC
    ext["linvel"][n:] = (0, 0, 4.0)
    ext["pos"][n] = (-7.7, 0.5, -0.4)
    ext["shape_type"][n] = scenes.SHAPE_SPHERE; ext["shape_param"][n] = (0.5, 0, 0, 0)
    ext["pos"][n + 1] = (-9.0, 0.3, -0.4)
    ext["shape_type"][n + 1] = scenes.SHAPE_CAPSULE; ext["shape_param"][n + 1] = (0.3, 0.3, 0, 0)
    ext["pos"][n + 2] = (-6.4, 0.3, -0.4)
    ext["shape_type"][n + 2] = scenes.SHAPE_CYLINDER; ext["shape_param"][n + 2] = (0.3, 0.3, 0, 0)
    assert (n, n + 1, n + 2) == (SPHERE, CAPSULE, CYLINDER)
    return ext


def _cfg(**kw):
    return edyn_amd.init_config(num_solver_velocity_iterations=10, **kw)


def _pair(scene, shards, **kw):
    """(the single context - None for shards == 0 -, the world): the same scene on both."""
    n = len(scene["kind"])
    if shards == 0:
        w = edyn_amd.World(_cfg(max_bodies=n + 64, **kw)); w.set_scene(scene); scenes.apply_figure_settings(w, scene)
        return w
    mw = MultiWorld(_cfg(**kw), devices=[0] * shards)
    mw.set_scene(scene)
    return mw


def _rolling_materials(w):
    """Rolling and spinning friction on the ground and the three rollers, soft boxes in the pile they start beside."""
    w.set_material_extras(0, spin=[0.05], roll=[0.005])
    w.set_material_extras(SPHERE, spin=[0.1, 0.02, 0.03], roll=[0.02, 0.015, 0.012])
    w.set_material_extras(SOFT.start, stiffness=np.full(64, STIFF, np.float32), damping=np.full(64, DAMP, np.float32))


def _snapshot(w, events=False):
    s = {"state": [a.copy() for a in w.get_state()], "manifolds": w.get_manifolds().copy(), "extras": w.get_point_extras().copy()}
    if events:
        s["events"] = w.get_contact_events().copy()
        s["ids"] = w.get_point_ids().copy()
    return s


def _idless(ev):
    a = np.stack([ev["step"].astype(np.int64), ev["type"].astype(np.int64), ev["body"][:, 0].astype(np.int64), ev["body"][:, 1].astype(np.int64)], 1) \
        if len(ev) else np.zeros((0, 4), np.int64)
    return a[np.lexsort(a.T[::-1])]


def _same(got, want, what, live=None):
    for a, b in zip(got["state"], want["state"]):
        assert np.array_equal(a if live is None else a[live], b if live is None else b[live]), (what, "state")
    gm, sm = got["manifolds"], want["manifolds"]
    assert len(gm) == len(sm), (what, len(gm), len(sm))
    for f in ("body", "num_points", "colour"):
        assert np.array_equal(gm[f], sm[f]), (what, f)
    for f in _capi.POINT_DTYPE.names:
        assert np.array_equal(gm["pt"][f], sm["pt"][f]), (what, f)
    assert got["extras"].shape == want["extras"].shape and got["extras"].dtype == want["extras"].dtype, what
    assert np.array_equal(got["extras"], want["extras"]), (what, "point extras")
    if "events" in want:
        assert np.array_equal(_idless(got["events"]), _idless(want["events"])), (what, "events")
        assert got["ids"].shape == want["ids"].shape and np.array_equal(got["ids"] == 0, want["ids"] == 0), (what, "point ids")


# ---- 1. rolling across the cut -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rolling_reference():
    w = _pair(_bridge_scene(), 0, contact_events=True)
    _rolling_materials(w)
    out = []
    for k in MIXED_120:
        w.step_simulation(k)
        out.append(_snapshot(w, events=True))
    return out


@pytest.mark.parametrize("shards", SHARDS)
def test_rolling_across_the_cut(shards):
    ref = _rolling_reference()
    mw = _pair(_bridge_scene(), shards, contact_events=True)
    _rolling_materials(mw)
    seen, after = 0, []     # the calls right after one in which the world re-partitioned, with the steps taken since that call began
    pending = None
    for call, k in enumerate(MIXED_120):
        mw.step_simulation(k)
        got = _snapshot(mw, events=True)
        _same(got, ref[call], (shards, call))
        if pending is not None:
            after.append((got, pending + k))
            pending = None
        reps = mw.get_stats()["repartitions"]
        if reps > seen:
            seen, pending = reps, k
    rolling = ref[-1]["extras"]
    assert (np.abs(rolling[:, :, 0:3]).max() > 0) and (rolling[:, :, 3].max() > 0), "nothing rolls in this scene"
    soft = ref[-1]["extras"][:, :, 5]
    assert ((soft > 0) & (soft < LARGE)).any(), "no soft contact in this scene"
    if shards >= 2:
        st = mw.get_stats()
        assert st["repartitions"] >= 1 and st["extras_carries"] >= 1, st
        carried_rolling = 0
        for got, steps in after:
            old = got["manifolds"]["pt"]["lifetime"] > steps           # created before the re-partition: carried through it
            x = got["extras"]
            carried_rolling += int((old & (np.abs(x[:, :, 0:3]).max(axis=2) > 0) & (x[:, :, 3] > 0)).sum())
        assert after and carried_rolling >= 1, "no carried point with a rolling or spinning impulse and a mixed roll coefficient"
    mw.close()


# ---- 2. the mix of a point's creation survives the move ------------------------------------------------------------------------------
def _sliding_piles():
    """mini_piles(2, 1) with the top layer of either pile pushed sideways: points keep being made while the layers slide."""
    sc = scenes.mini_piles(2, 1)
    for t in range(2):
        sc["linvel"][1 + 64 * t + 48:1 + 64 * (t + 1)] = (1.5, 0, 0.5)
    return sc


def _piles_run(w, repartition):
    """Materials, 12 steps, other materials on bodies in contact, (forced re-partitions), 12 more steps: a snapshot per phase."""
    w.set_material_extras(0, spin=[0.05], roll=[0.08])
    w.set_material_extras(1, spin=np.full(128, 0.04, np.float32), roll=np.full(128, 0.06, np.float32),
                          stiffness=np.where(np.arange(128) < 64, STIFF, 1e18).astype(np.float32), damping=np.where(np.arange(128) < 64, DAMP, 1e18).astype(np.float32))
    out = []
    w.step_simulation(12)
    out.append(_snapshot(w))
    w.set_material_extras(0, spin=[0.2], roll=[0.0])
    w.set_material_extras(1, spin=np.full(128, 0.3, np.float32), roll=np.full(128, 0.01, np.float32))     # (stiff again)
    out.append(_snapshot(w))
    if repartition:
        for _ in range(2):
            w.repartition()
            out.append(_snapshot(w))
    for _ in range(4):
        w.step_simulation(3)
        out.append(_snapshot(w))
    return out


@functools.lru_cache(maxsize=None)
def _piles_reference():
    return _piles_run(_pair(_sliding_piles(), 0), False)


@pytest.mark.parametrize("shards", SHARDS)
def test_creation_time_mix_survives_the_move(shards):
    ref = _piles_reference()
    mw = _pair(_sliding_piles(), shards)
    before = mw.get_stats()
    got = _piles_run(mw, True)
    st = mw.get_stats()
    assert st["repartitions"] == before["repartitions"] + 2 and st["extras_carries"] == 2, st
    _same(got[0], ref[0], (shards, "before the change"))
    _same(got[1], ref[1], (shards, "materials changed"))
    for k in (2, 3):    # forced re-partitions alone change nothing: the points keep the mix they were created with, not today's
        _same(got[k], got[1], (shards, "re-partition", k))
    for k in range(4):
        _same(got[4 + k], ref[2 + k], (shards, "stepping on", k))
    old = ref[1]["extras"]
    assert (old[:, :, 3] == np.float32(0.08)).any() and ((old[:, :, 5] > 0) & (old[:, :, 5] < LARGE)).any(), "the old mix is not in the scene"
    last, life = ref[-1]["extras"], ref[-1]["manifolds"]["pt"]["lifetime"]
    live = np.arange(4)[None, :] < ref[-1]["manifolds"]["num_points"][:, None]
    assert (live & (life > 12) & (last[:, :, 3] == np.float32(0.08))).any(), "no point kept its old mix"
    assert (live & (life <= 12) & (last[:, :, 4] == np.float32(0.3))).any(), "no new point with the new mix"
    mw.close()


# ---- 3. ids and the mix table --------------------------------------------------------------------------------------------------------
def _mix_setup(w):
    ids = np.zeros(388, np.uint32)
    ids[1:385] = 1 + (np.arange(384) % 2)           # the boxes: ids 1 and 2 alternately
    ids[385:] = (2, 1, 2)
    w.set_material_ids(0, ids)                      # the ground: id 0
    w.insert_material_mixing(0, 1, friction=0.4, roll=0.05)
    w.insert_material_mixing(1, 0, friction=0.45, spin=0.02)                  # both orders
    w.insert_material_mixing(1, 2, restitution=0.25, friction=0.3)            # one order only; the restitution solver runs


@functools.lru_cache(maxsize=None)
def _mix_reference():
    w = _pair(_bridge_scene(), 0)
    _mix_setup(w)
    out, done = [], 0
    for k in MIXED_90:
        w.step_simulation(k)
        done += k
        if done == 30:
            w.insert_material_mixing(0, 2, friction=0.6, spin=0.1, roll=0.07, stiffness=STIFF, damping=DAMP)
        out.append(_snapshot(w))
    return out


@pytest.mark.parametrize("shards", SHARDS)
def test_ids_and_the_mix_table(shards):
    ref = _mix_reference()
    mw = _pair(_bridge_scene(), shards)
    _mix_setup(mw)
    done = 0
    for call, k in enumerate(MIXED_90):
        mw.step_simulation(k)
        done += k
        if done == 30:
            edits = mw.get_edit_stats()
            mw.insert_material_mixing(0, 2, friction=0.6, spin=0.1, roll=0.07, stiffness=STIFF, damping=DAMP)
            st = mw.get_edit_stats()
            assert (st["edits"], st["in_place"]) == (edits["edits"] + 1, edits["in_place"] + 1) and st["repartitions_by_edit"] == 0, st
        _same(_snapshot(mw), ref[call], (shards, call))
    fr = ref[-1]["manifolds"]["pt"]["friction"]
    assert all((fr == np.float32(v)).any() for v in (0.3, 0.6)) and ((fr == np.float32(0.4)) | (fr == np.float32(0.45))).any(), "mix entries unused"
    assert (ref[-1]["manifolds"]["pt"]["restitution"] == np.float32(0.25)).any(), "the entry with restitution is unused"
    if shards >= 2:
        st = mw.get_stats()
        assert st["repartitions"] >= 1 and st["extras_carries"] >= 1, st
    mw.close()


# ---- 4. edits ------------------------------------------------------------------------------------------------------------------------
def _new_bodies():
    """A sphere and a capsule dropped onto the pile of site 0 of mini_piles(2, 1), and a static box beside the pile of site 1."""
    s = scenes._empty(3)
    s["pos"][0] = (-4.0, 5.2, 0.3); s["shape_type"][0] = scenes.SHAPE_SPHERE; s["shape_param"][0] = (0.5, 0, 0, 0)
    s["pos"][1] = (-4.3, 6.4, -0.2); s["shape_type"][1] = scenes.SHAPE_CAPSULE; s["shape_param"][1] = (0.3, 0.3, 0, 0)
    s["kind"][2] = scenes.KIND_STATIC
    s["pos"][2] = (4.0 + 2.05 + 0.5, 0.5, 0.0); s["shape_type"][2] = scenes.SHAPE_BOX; s["shape_param"][2] = (0.5, 0.5, 0.5, 0)
    return s


def _edit_run(w, multi):
    w.set_material_extras(0, spin=[0.05], roll=[0.08])
    w.set_material_ids(1, np.full(64, 5, np.uint32))      # the pile the new bodies land on
    w.insert_material_mixing(5, 3, friction=0.7, roll=0.09)
    w.insert_material_mixing(3, 5, friction=0.7, roll=0.09)
    out = []
    w.step_simulation(10)
    first = w.add_scene(_new_bodies())
    first = first[0] if multi else first
    assert first == 129
    w.set_material_extras(first, spin=[0.1, 0.05, 0.0], roll=[0.2, 0.1, 0.3])
    w.set_material_ids(first, np.array([3, 0xFFFF, 3], np.uint32))
    w.set_material_extras(40, spin=[0.07, 0.07], roll=[0.03, 0.03], stiffness=[STIFF, STIFF], damping=[DAMP, DAMP])
    out.append(_snapshot(w))
    for _ in range(10):
        w.step_simulation(3)
        out.append(_snapshot(w))
    w.remove_bodies([first, 40])     # two bodies with materials
    for _ in range(5):
        w.step_simulation(2)
        out.append(_snapshot(w))
    return out


@functools.lru_cache(maxsize=None)
def _edit_reference():
    return _edit_run(_pair(scenes.mini_piles(2, 1), 0), False)


@pytest.mark.parametrize("shards", SHARDS)
def test_edits(shards):
    ref = _edit_reference()
    mw = _pair(scenes.mini_piles(2, 1), shards)
    got = _edit_run(mw, True)
    live = np.ones(132, bool)
    for k, (g, r) in enumerate(zip(got, ref)):
        if k == 11:
            live[[129, 40]] = False
        _same(g, r, (shards, k), live)
    x = ref[10]["extras"]
    assert (x[:, :, 3] == np.float32(0.09)).any() and (np.abs(x[:, :, 0:3]).max() > 0), "the new bodies' materials are unused"
    mw.close()


# ---- 5. arguments and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_arguments_and_refusals(shards):
    L = _capi.lib()
    scene = _sliding_piles()
    n = len(scene["kind"])
    mw = _pair(scene, shards)
    one = np.array([0.1], np.float32)
    ids = np.array([1], np.uint32)
    m6 = np.array([0, 0.5, 0, 0, 1e18, 1e18], np.float32)
    for running in (False, True):
        assert L.edynhip_world_set_material_extras(mw._h, n, 1, one.ctypes.data, None, None, None) == ERR_INVALID
        assert b"out of bounds" in L.edynhip_world_last_error(mw._h)
        assert L.edynhip_world_set_material_extras(mw._h, 0xFFFFFFFF, 2, one.ctypes.data, None, None, None) == ERR_INVALID
        assert L.edynhip_world_set_material_ids(mw._h, n - 1, 2, ids.ctypes.data) == ERR_INVALID
        assert b"edynhip_world_set_material_ids" in L.edynhip_world_last_error(mw._h)
        assert L.edynhip_world_set_material_ids(mw._h, 0, 1, None) == ERR_INVALID
        assert L.edynhip_world_set_material_ids(mw._h, 0, 1, np.array([0x10000], np.uint32).ctypes.data) == ERR_INVALID
        assert L.edynhip_world_set_material_extras(mw._h, 0, 1, (-one).ctypes.data, None, None, None) == ERR_INVALID
        assert L.edynhip_world_set_material_extras(mw._h, 0, 1, None, None, (0 * one).ctypes.data, None) == ERR_INVALID
        assert L.edynhip_world_insert_material_mixing(mw._h, 0xFFFF, 0, m6.ctypes.data) == ERR_INVALID
        assert b"unassigned" in L.edynhip_world_last_error(mw._h)
        assert L.edynhip_world_insert_material_mixing(mw._h, 0, 1, None) == ERR_INVALID
        assert L.edynhip_world_set_material_extras(mw._h, n, 0, None, None, None, None) == 0     # an empty range at the end
        if not running:
            mw.step_simulation(5)
    # nothing above changed the world: it is the single context without materials, and no extras were carried
    w = _pair(scene, 0)
    w.step_simulation(5)
    _same(_snapshot(mw), _snapshot(w), (shards, "untouched"))
    mw.repartition()
    assert mw.get_stats()["extras_carries"] == 0, "a world without materials carried point extras"
    _same(_snapshot(mw), _snapshot(w), (shards, "untouched, re-partitioned"))
    # all arrays NULL: the defaults again
    for x in (mw, w):
        x.set_material_extras(0, spin=[0.2], roll=[0.1])
        x.set_material_extras(1, spin=np.full(64, 0.07, np.float32), stiffness=np.full(64, STIFF, np.float32), damping=np.full(64, DAMP, np.float32))
        x.step_simulation(3)
    assert L.edynhip_world_set_material_extras(mw._h, 0, n, None, None, None, None) == 0
    assert L.edynhip_set_material_extras(w._h, 0, n, None, None, None, None) == 0
    for x in (mw, w):
        x.step_simulation(3)
    got, want = _snapshot(mw), _snapshot(w)
    _same(got, want, (shards, "defaults restored"))
    life = want["manifolds"]["pt"]["lifetime"]
    live = np.arange(4)[None, :] < want["manifolds"]["num_points"][:, None]
    fresh = live & (life <= 2)      # (made since the defaults came back, if any was)
    assert (want["extras"][fresh][:, 3:] == np.array([0, 0, LARGE, LARGE], np.float32)).all()
    # the points made before outlive their bodies' materials, also through a re-partition of shards none of whose bodies has one now
    assert (live & (want["extras"][:, :, 4] > 0)).any() and ((want["extras"][:, :, 5] > 0) & (want["extras"][:, :, 5] < LARGE)).any()
    mw.repartition()
    _same(_snapshot(mw), want, (shards, "defaults restored, re-partitioned"))
    for x in (mw, w):
        x.step_simulation(3)
    got, want = _snapshot(mw), _snapshot(w)
    _same(got, want, (shards, "defaults restored, re-partitioned, stepped"))
    # capacity: too small a table is refused, the count still comes back
    cnt = C.c_uint32(0)
    assert L.edynhip_world_get_point_extras(mw._h, None, 0, C.byref(cnt)) == 0 and cnt.value == len(want["manifolds"]) > 1
    out = np.zeros((cnt.value, 4, 7), np.float32)
    k = C.c_uint32(0)
    assert L.edynhip_world_get_point_extras(mw._h, out.ctypes.data, cnt.value - 1, C.byref(k)) == ERR_CAPACITY and k.value == cnt.value
    assert not out.any()
    assert L.edynhip_world_get_point_extras(mw._h, out.ctypes.data, cnt.value, C.byref(k)) == 0 and np.array_equal(out, want["extras"])
    # a shard context stays the world's: the single-context calls refuse it
    for r in range(shards):
        ctx = C.c_void_p(L.edynhip_world_context(mw._h, r))
        assert ctx
        assert L.edynhip_set_material_extras(ctx, 0, 1, one.ctypes.data, None, None, None) == ERR_UNSUPPORTED
        assert L.edynhip_set_material_ids(ctx, 0, 1, ids.ctypes.data) == ERR_UNSUPPORTED
        assert L.edynhip_insert_material_mixing(ctx, 0, 1, m6.ctypes.data) == ERR_UNSUPPORTED
        assert L.edynhip_get_point_extras(ctx, out.ctypes.data, cnt.value, C.byref(k)) == ERR_UNSUPPORTED
        assert b"multi-device world" in L.edynhip_last_error(ctx)
    _same(_snapshot(mw), want, (shards, "after the refusals"))
    mw.close()


# ---- 6. kernel edges -----------------------------------------------------------------------------------------------------------------
def _edge_scene(count):
    """`count` bodies resting on the ground, one manifold each, far enough apart to be islands of their own: spheres (1 point), capsules
    on their sides (2), boxes (4) and boxes that hang over the corner of a static block (3: the corner of the block's top face cuts a
    triangle out of the box's bottom face)."""
    blocks = count // 4
    s = scenes._empty(1 + count + blocks)
    scenes._add_plane(s)
    for k in range(count):
        i = 1 + k
        x, z = 3.0 * (k % 20), 3.0 * (k // 20)
        s["pos"][i] = (x, 0.5, z)
        what = k % 4
        if what == 0:
            s["shape_type"][i] = scenes.SHAPE_SPHERE; s["shape_param"][i] = (0.5, 0, 0, 0)
        elif what == 1:
            s["shape_type"][i] = scenes.SHAPE_CAPSULE; s["shape_param"][i] = (0.3, 0.4, 0, 0); s["pos"][i, 1] = 0.3
        elif what == 2:
            s["shape_type"][i] = scenes.SHAPE_BOX; s["shape_param"][i] = (0.5, 0.5, 0.5, 0)
        else:   # a box on a block twice as high as the gap below it, turned by 45 degrees, its centre above the block's corner region
            b = 1 + count + k // 4
            s["kind"][b] = scenes.KIND_STATIC
            s["shape_type"][b] = scenes.SHAPE_BOX; s["shape_param"][b] = (0.5, 0.5, 0.5, 0); s["pos"][b] = (x, 0.5, z)
            s["shape_type"][i] = scenes.SHAPE_BOX; s["shape_param"][i] = (0.5, 0.5, 0.5, 0)
            s["pos"][i] = (x + 0.75, 1.5, z + 0.75)
            s["orn"][i] = (0, np.sin(np.pi / 8), 0, np.cos(np.pi / 8))
    return s


@functools.lru_cache(maxsize=None)
def _edge_reference(count):
    w = _pair(_edge_scene(count), 0)
    w.set_material_extras(0, spin=np.full(1 + count, 0.05, np.float32), roll=np.full(1 + count, 0.08, np.float32))
    w.step_simulation(3)
    return _snapshot(w)


@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("count", [0, 1, 257])
def test_kernel_edges(shards, count):
    """The gather and the inject at the sizes where they can go wrong - no manifold, one, 257 = one past a block of 256 (every body of
    the scene has one manifold; with one shard all 257 are one context's) - over manifolds of 1, 2,
    3 and 4 points: a forced re-partition gathers every row, rebuilds the arrays through edynhip_set_manifolds - which mixes every point
    afresh from the bodies' materials, changed below - and injects the rows; the read-back gathers again."""
    want = _edge_reference(count)
    mw = _pair(_edge_scene(count), shards)
    mw.set_material_extras(0, spin=np.full(1 + count, 0.05, np.float32), roll=np.full(1 + count, 0.08, np.float32))
    mw.step_simulation(3)
    got = _snapshot(mw)
    _same(got, want, (shards, count))
    num = want["manifolds"]["num_points"]
    if count == 0:
        assert len(num) == 0 and got["extras"].shape == (0, 4, 7)
    elif count == 1:
        assert len(num) == 1
    else:
        assert len(num) == 257 and {1, 2, 3, 4} <= set(num.tolist()), np.bincount(num)
        dead = np.arange(4)[None, :] >= num[:, None]
        assert not want["extras"][dead].any() and (want["extras"][~dead][:, 3] == np.float32(0.08)).all()
        assert np.abs(want["extras"][:, :, 0:3]).max() > 0
    mw.set_material_extras(0, spin=np.full(1 + count, 0.5, np.float32), roll=np.full(1 + count, 0.6, np.float32))   # today's materials
    for _ in range(2):
        mw.repartition()
        _same(_snapshot(mw), want, (shards, count, "gather, inject, gather"))
    assert mw.get_stats()["extras_carries"] == (2 if count else 0)
    mw.close()
