"""Raycast and AABB queries on a multi-device world (edynhip_world_raycast / edynhip_world_query_aabb, MultiWorld.raycast /
.query_aabb): 2 and 3 shards on device 0. The answer must be bit for bit what ONE context holding the whole scene returns - against
the reference's recorded results on the fixture scene, against a single World through a re-partition (tree, ignore list, brute
force, all three categories), for ties in fraction between bodies that different shards answer for, and through the device entries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd.multi import MultiWorld

import query_ref
import test_raycast_golden as trg
from test_multirank_gloo import _bridge_scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_query_aabb as mq   # noqa: E402
import make_raycast as mr      # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -4, -6
CATS = ("procedural", "non_procedural", "islands")
SHARDS = [2, 3]


def _cfg(**kw):
    return edyn_amd.init_config(num_solver_velocity_iterations=10, **kw)


def _pair(scene, shards, **kw):
    """One context and a multi-device world (all shards on device 0) holding the same scene."""
    single = edyn_amd.World(_cfg(**kw)); single.set_scene(scene); scenes.apply_figure_settings(single, scene)
    mw = MultiWorld(_cfg(**kw), devices=[0] * shards)
    mw.set_scene(scene)
    return single, mw


def _dynamic_shaped(scene):
    dyn = np.asarray(scene["kind"]) == scenes.KIND_DYNAMIC
    shaped = np.asarray(scene["shape_type"]) != scenes.SHAPE_NONE
    return dyn & shaped, ~dyn & shaped


# ---- 1. golden: the reference's own results on the fixture scene ----------------------------------------------------------------
@pytest.fixture(scope="module", params=SHARDS)
def fixture_world(request):
    s = mr.scene()
    mw = MultiWorld(edyn_amd.init_config(gravity=(0.0, 0.0, 0.0)), devices=[0] * request.param)
    mw.set_scene(s)
    mw.step_simulation(1)
    yield s, mw, request.param
    mw.close()


def test_fixture_partition_spreads_the_dynamic_bodies(fixture_world):
    s, mw, shards = fixture_world
    part = mw.get_partition()
    dyn = np.asarray(s["kind"]) == scenes.KIND_DYNAMIC
    assert np.all(part[~dyn] == -1)
    assert set(part[dyn].tolist()) == set(range(shards))


@pytest.mark.parametrize("kind", mr.KINDS)
def test_world_equals_reference_raycast(fixture_world, kind):
    s, mw, _ = fixture_world
    p0, p1 = mr.rays(kind, s)
    fx = np.load(os.path.join(os.path.dirname(mr.__file__), f"raycast_{kind}.npz"))
    assert str(fx["rays_sha256"]) == mr.digest(p0, p1) and str(fx["scene_sha256"]) == mr.scene_digest(s)
    ref = fx["result"]
    dev = mw.raycast(p0, p1)
    ok = trg._same(dev, ref)
    bad = np.flatnonzero(~ok)
    ties = 0
    for i in bad:   # an exact tie: with the device's choice ignored, the reference's body comes out
        if dev["fraction"][i] != ref["fraction"][i] or dev["body"][i] == NONE:
            continue
        again = mw.raycast(p0[i], p1[i], ignore=[int(dev["body"][i])])
        if trg._same(again, ref[i:i + 1])[0]:
            ties += 1
    assert ties == len(bad), (kind, len(bad) - ties, [(int(i), dev[i], ref[i]) for i in bad[:5]])
    hit = ref["entity"] != NONE
    assert hit.sum() > 2000
    if kind in ("inside", "parallel"):
        assert (ref["variant"][hit] == 4).sum() > 1000   # polyhedra reached


@pytest.mark.parametrize("which", mq.SETS)
def test_world_equals_the_reference_tree(fixture_world, which):
    s, mw, _ = fixture_world
    fx = np.load(os.path.join(os.path.dirname(mq.__file__), f"query_aabb_{which}.npz"))
    q = mq.queries(which, s, fx["aabb"])
    assert str(fx["scene_sha256"]) == mr.scene_digest(s) and str(fx["queries_sha256"]) == mr.digest(q)
    for cat in mq.CATEGORIES:
        for brute in (False, True):
            off, ids = mw.query_aabb(q, cat, brute_force=brute)
            assert np.array_equal(off, fx[cat + "_offsets"]) and np.array_equal(ids, fx[cat + "_ids"]), (which, cat, brute)


# ---- 2. equal to one context through a re-partition -------------------------------------------------------------------------------
RAYS_PER_KIND = 820   # x 5 kinds = 4 100 rays


def _rays_for(scene, pos, orn):
    """The kinds of make_raycast.rays on the scene's current state; the two kinds that fill a fixed volume are rescaled to the scene."""
    s = dict(scene); s["pos"] = pos; s["orn"] = orn
    ext = np.abs(pos[np.asarray(scene["shape_type"]) != scenes.SHAPE_PLANE]).max(0) + 2.0
    scale = np.float32([ext[0] / 10.0, 1.0, ext[2] / 10.0])
    out0, out1 = [], []
    for kind in mr.KINDS:
        p0, p1 = mr.rays(kind, s, n=RAYS_PER_KIND)
        if kind in ("random", "plane"):
            p0, p1 = p0 * scale, p1 * scale
        out0.append(p0); out1.append(p1)
    return np.concatenate(out0).astype(np.float32), np.concatenate(out1).astype(np.float32)


def _boxes_for(aabb, n, seed):
    """Body-sized and larger boxes over the scene; box 0 holds the whole scene, box 1 nothing, box 2 is NaN."""
    rng = np.random.default_rng(seed)
    lo, hi = aabb[:, :3].min(0), aabb[:, 3:].max(0)
    c = rng.uniform(lo - 1, hi + 1, size=(n, 3))
    h = np.where(rng.integers(0, 4, n)[:, None] < 3, rng.uniform(0.2, 0.8, (n, 3)), rng.uniform(2.0, 6.0, (n, 3)))
    q = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    q[0] = np.float32([-1e6] * 3 + [1e6] * 3)
    q[1] = q[1] + np.float32(1e4)
    q[2] = np.nan
    return q


def _finite_boxes(single, scene):
    aabb = single.get_derived()[0]
    st = np.asarray(scene["shape_type"])
    return aabb[(st != scenes.SHAPE_NONE) & (st != scenes.SHAPE_PLANE)]


def _compare_all(single, mw, scene, seed, what):
    pos, orn = single.get_state()[:2]
    p0, p1 = _rays_for(scene, pos, orn)
    assert len(p0) >= 4096
    dyn, _ = _dynamic_shaped(scene)
    ignore = np.flatnonzero(dyn)[::3].tolist() + [0, len(dyn) - 1, len(dyn) + 7]   # dynamic bodies of every shard, the plane, one out of range
    hits = 0
    for kw in ({}, {"ignore": ignore}, {"brute_force": True}):
        a, b = single.raycast(p0, p1, **kw), mw.raycast(p0, p1, **kw)
        assert a.tobytes() == b.tobytes(), (what, kw and list(kw)[0], int(np.sum(a != b)))
        hits += int((a["body"] != NONE).sum())
    assert hits > 1000
    q = _boxes_for(_finite_boxes(single, scene), 512, seed)
    for cat in CATS:
        for brute in (False, True):
            a, b = single.query_aabb(q, cat, brute_force=brute), mw.query_aabb(q, cat, brute_force=brute)
            assert np.array_equal(a[0], b[0]), (what, cat, brute, "offsets")
            assert np.array_equal(a[1], b[1]), (what, cat, brute, "ids")
            assert a[0][1] - a[0][0] > 0 and a[0][2] == a[0][1] and a[0][3] == a[0][2]   # everything, nothing, NaN


@pytest.mark.parametrize("shards", SHARDS)
def test_world_equals_one_context_through_a_repartition(shards):
    scene = _bridge_scene(along="z")
    single, mw = _pair(scene, shards)
    _compare_all(single, mw, scene, 1000, "described, not stepped")
    for k in range(90):
        single.step_simulation(1); mw.step_simulation(1)
        _compare_all(single, mw, scene, k, k)
    for x, y in zip(single.get_state(), mw.get_state()):
        assert np.array_equal(x, y)   # the queries changed nothing a step computes
    assert mw.get_stats()["repartitions"] >= 1
    mw.close()


# ---- 3. every body once -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_every_body_is_answered_once(shards):
    scene = _bridge_scene(along="z")
    single, mw = _pair(scene, shards)
    single.step_simulation(40); mw.step_simulation(40)
    everything = np.float32([[-1e6] * 3 + [1e6] * 3])
    dyn, rest = _dynamic_shaped(scene)
    assert scenes.SHAPE_PLANE in np.asarray(scene["shape_type"])[rest]
    off, ids = mw.query_aabb(everything, "procedural")
    assert np.array_equal(ids, np.flatnonzero(dyn)) and off.tolist() == [0, int(dyn.sum())]
    off, ids = mw.query_aabb(everything, "non_procedural")
    assert np.array_equal(ids, np.flatnonzero(rest)) and len(set(ids.tolist())) == len(ids)
    labels = single.get_derived()[2]
    off, ids = mw.query_aabb(everything, "islands")
    assert np.array_equal(ids, np.unique(labels[dyn]))
    assert 1 < len(ids) < dyn.sum()
    mw.close()


# ---- 4. ties in fraction between bodies of different shards ----------------------------------------------------------------------
def _row_of_boxes(count=16):
    """Unit boxes side by side along x, identity orientation, centres at integers (every face on a multiple of 0.5), alternately static
    and dynamic, zero gravity: the top faces are coplanar, a vertical ray on a seam meets two boxes at the same fraction."""
    s = scenes._empty(count)
    for i in range(count):
        s["kind"][i] = scenes.KIND_STATIC if i % 2 == 0 else scenes.KIND_DYNAMIC
        s["pos"][i] = (float(i), 0.0, 0.0)
        s["shape_type"][i] = scenes.SHAPE_BOX
        s["shape_param"][i] = (0.5, 0.5, 0.5, 0)
    return s


@pytest.mark.parametrize("shards", SHARDS)
def test_ties_between_bodies_of_different_shards(shards):
    scene = _row_of_boxes()
    n = len(scene["kind"])
    single, mw = _pair(scene, shards, gravity=(0.0, 0.0, 0.0))
    part = mw.get_partition()
    assert np.all(part[0::2] == -1), "static boxes are replicated: shard 0 answers for them"
    assert (part[1::2] > 0).any(), "a static box's dynamic neighbour is answered by another shard"
    seams = np.arange(n - 1, dtype=np.float32) + np.float32(0.5)
    zs = np.float32([0.0, 0.25, -0.5, 0.5])
    p0 = np.float32([(x, 2.0, z) for x in seams for z in zs])
    p1 = p0 * np.float32([1, -1, 1])
    first = single.raycast(p0, p1)
    assert (first["body"] != NONE).all()
    true_ties = cross = 0
    for i in range(len(p0)):   # the condition: on ONE context, ignoring the winner gives another body at a bit-equal fraction
        again = single.raycast(p0[i], p1[i], ignore=[int(first["body"][i])])[0]
        if again["body"] != NONE and again["body"] != first["body"][i] and again["fraction"].tobytes() == first["fraction"][i].tobytes():
            true_ties += 1
            a, b = int(first["body"][i]), int(again["body"])
            owner = [0 if part[x] < 0 else int(part[x]) for x in (a, b)]
            cross += owner[0] != owner[1]
    assert true_ties >= 1, "no seam ray is a true tie on the single context: change the geometry"
    assert cross >= 1, "no tie is between bodies that different shards answer for"
    for kw in ({}, {"brute_force": True}):
        got = mw.raycast(p0, p1, **kw)
        assert got.tobytes() == single.raycast(p0, p1, **kw).tobytes(), (kw, np.flatnonzero(got["body"] != first["body"])[:8])
    # and with the winners ignored: the other body of every tie
    ign = np.unique(first["body"]).tolist()
    assert mw.raycast(p0, p1, ignore=ign).tobytes() == single.raycast(p0, p1, ignore=ign).tobytes()
    mw.close()


# ---- 5. device entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_device_entries_equal_the_host_entries(shards):
    import torch
    scene = _bridge_scene(along="z")
    single, mw = _pair(scene, shards)
    single.step_simulation(20); mw.step_simulation(20)
    dev = torch.device("cuda", 0)
    pos, orn = single.get_state()[:2]
    p0, p1 = _rays_for(scene, pos, orn)
    n = len(p0)
    d0 = torch.zeros((n, 4), dtype=torch.float32, device=dev); d0[:, :3] = torch.from_numpy(p0).to(dev)
    d1 = torch.zeros((n, 4), dtype=torch.float32, device=dev); d1[:, :3] = torch.from_numpy(p1).to(dev)
    out = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for kw in ({}, {"ignore": [1, 2, 70, 200]}, {"brute_force": True}):
        mw.raycast_device(n, d0.data_ptr(), d1.data_ptr(), out.data_ptr(), **kw)
        got = out.cpu().numpy().view(_capi.RAYCAST_HIT_DTYPE).reshape(-1)
        assert got.tobytes() == mw.raycast(p0, p1, **kw).tobytes() == single.raycast(p0, p1, **kw).tobytes()
    q = _boxes_for(_finite_boxes(single, scene), 512, 5)
    boxes = torch.zeros((2 * len(q), 4), dtype=torch.float32, device=dev)
    boxes[:, :3] = torch.from_numpy(q.reshape(-1, 3)).to(dev)
    SENTINEL = 0x6B6B6B6B
    for cat in CATS:
        host = mw.query_aabb(q, cat)
        tot = int(host[0][-1])
        assert tot > 8
        for capacity in (tot, tot // 2, 0):
            off = torch.zeros(len(q) + 1, dtype=torch.int32, device=dev)
            ids = torch.full((tot,), SENTINEL, dtype=torch.int32, device=dev)
            total = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            mw.query_aabb_device(len(q), boxes.data_ptr(), off.data_ptr(), ids.data_ptr() if capacity else None, capacity, total.data_ptr(), category=cat)
            assert int(total.cpu().numpy().view(np.uint32)[0]) == tot                      # total and offsets are complete whatever fits
            assert np.array_equal(off.cpu().numpy().view(np.uint32), host[0])
            got = ids.cpu().numpy().view(np.uint32)
            assert np.all(got[capacity:] == SENTINEL), (cat, capacity)                      # nothing at or beyond capacity
            fits = host[0][1:] <= capacity                                                  # queries that end inside the buffer
            for i in np.flatnonzero(fits):
                assert np.array_equal(got[host[0][i]:host[0][i + 1]], host[1][host[0][i]:host[0][i + 1]]), (cat, capacity, int(i))
        # the host entry with a buffer that is too small: EDYNHIP_ERR_CAPACITY, offsets and total complete
        b = np.ascontiguousarray(q)
        off = np.zeros(len(q) + 1, np.uint32); small = np.full(tot // 2, SENTINEL, np.uint32); total = C.c_uint32(0)
        rc = mw._L.edynhip_world_query_aabb(mw._h, _capi.QUERY_CATEGORIES[cat], len(b), b.ctypes.data, 0, off.ctypes.data, small.ctypes.data, len(small), C.byref(total))
        assert rc == ERR_CAPACITY and total.value == tot and np.array_equal(off, host[0])
    mw.close()


# ---- 6. arguments, and the shard contexts stay closed ------------------------------------------------------------------------------
def test_bad_arguments_and_shard_contexts():
    mw = MultiWorld(edyn_amd.init_config(), devices=(0, 0))
    mw.set_scene(scenes.mini_piles(2, 2))
    L = mw._L
    p = np.float32([[0, 5, 0]]); q = np.float32([[0, -5, 0]]); out = np.zeros(1, _capi.RAYCAST_HIT_DTYPE)
    box = np.float32([[-1, -1, -1, 1, 1, 1]]); off = np.zeros(2, np.uint32); total = C.c_uint32(0)
    # a world that has been described but not stepped answers (it builds its shards first)
    assert L.edynhip_world_raycast(mw._h, 1, p.ctypes.data, q.ctypes.data, 0, None, 0, out.ctypes.data) == 0
    assert out["body"][0] != NONE
    assert L.edynhip_world_raycast(mw._h, 0, None, None, 0, None, 0, None) == 0
    assert L.edynhip_world_query_aabb(mw._h, 0, 0, None, 0, off.ctypes.data, None, 0, C.byref(total)) == 0 and total.value == 0 and off[0] == 0
    assert L.edynhip_world_raycast(mw._h, 1, p.ctypes.data, q.ctypes.data, 0, None, 2, out.ctypes.data) == ERR_INVALID
    assert L.edynhip_world_raycast(mw._h, 1, None, q.ctypes.data, 0, None, 0, out.ctypes.data) == ERR_INVALID
    assert L.edynhip_world_raycast(mw._h, 1, p.ctypes.data, q.ctypes.data, 1, None, 0, out.ctypes.data) == ERR_INVALID
    assert L.edynhip_world_query_aabb(mw._h, 0, 1, box.ctypes.data, 4, off.ctypes.data, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_world_query_aabb(mw._h, 3, 1, box.ctypes.data, 0, off.ctypes.data, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_world_query_aabb(mw._h, 0, 1, None, 0, off.ctypes.data, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_world_query_aabb(mw._h, 0, 1, box.ctypes.data, 0, None, None, 0, C.byref(total)) == ERR_INVALID
    mw.step_simulation(1)
    for shard in (0, 1):
        ctx = L.edynhip_world_context(mw._h, shard)
        assert ctx
        assert L.edynhip_raycast(ctx, 1, p.ctypes.data, q.ctypes.data, 0, None, 0, out.ctypes.data) == ERR_UNSUPPORTED
        assert L.edynhip_raycast_device(ctx, 1, p.ctypes.data, q.ctypes.data, 0, None, 0, out.ctypes.data) == ERR_UNSUPPORTED
        assert L.edynhip_query_aabb(ctx, 0, 1, box.ctypes.data, 0, off.ctypes.data, None, 0, C.byref(total)) == ERR_UNSUPPORTED
        assert L.edynhip_query_aabb_device(ctx, 0, 1, box.ctypes.data, 0, off.ctypes.data, None, 0, off.ctypes.data) == ERR_UNSUPPORTED
    mw.close()
