"""AABB queries on the device (edynhip_query_aabb / World.query_aabb): the reference's recorded dynamic_tree results on the fixture scene,
the query tree against the brute-force walk and against the definition in numpy (tests/query_ref.py) on the device's own AABBs, island
queries, the capacity protocol, the device entry point, and that a query changes nothing a later step or raycast computes. Every
comparison is exact equality of integer arrays."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd.world import EdynHipError

import bplayouts as bl
import query_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_query_aabb as mq   # noqa: E402
import make_raycast as mr      # noqa: E402

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -4, -6
CATS = ("procedural", "non_procedural")


def _world(scene, sleeping=False, max_bodies=0, gravity=None):
    kw = {} if gravity is None else {"gravity": gravity}
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, sleeping=sleeping,
                                            max_bodies=max_bodies, **kw))
    w.set_scene(scene)
    return w


def _queries(aabb, n, seed):
    """Mixed sizes in one batch: a body's size, ten times that, huge (every body), empty, inverted, NaN, and faces touching a fat box
    exactly with twins one ulp apart. aabb: the boxes of the shaped non-plane bodies."""
    rng = np.random.default_rng(seed)
    lo, hi = aabb[:, :3].min(0), aabb[:, 3:].max(0)
    c = rng.uniform(lo - 1, hi + 1, size=(n, 3))
    kind = rng.integers(0, 10, n)
    h = np.where(kind[:, None] < 5, rng.uniform(0.2, 0.8, (n, 3)), rng.uniform(3.0, 6.0, (n, 3)))
    q = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    pick = rng.integers(0, len(aabb), n)
    axis = rng.integers(0, 3, n)
    t, twin = mq.touching(aabb, pick, axis, rng.integers(0, 2, n), rng.random(n))
    q[kind == 8] = t[kind == 8]
    q[kind == 9] = twin[kind == 9]
    r = np.flatnonzero(kind == 7)[::2]   # inverted on one axis
    q[r, axis[r]], q[r, 3 + axis[r]] = q[r, 3 + axis[r]].copy(), q[r, axis[r]].copy()
    q[0:6] = np.float32([-1e6] * 3 + [1e6] * 3)          # every body
    q[6:12] = (q[6:12] + np.float32(1e4)).astype(np.float32)   # nothing
    q[12:18, rng.integers(0, 6, 6)] = np.nan
    q[12, :] = np.nan
    return q


def _masks(kind, shape, removed=()):
    shaped = np.asarray(shape) != scenes.SHAPE_NONE
    shaped[list(removed)] = False
    dyn = np.asarray(kind) == scenes.KIND_DYNAMIC
    return {"procedural": shaped & dyn, "non_procedural": shaped & ~dyn}


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "offsets", int(np.sum(a[0] != b[0])))
    assert np.array_equal(a[1], b[1]), (what, "ids")


def _check(w, kind, shape, q, what, removed=(), aabb=None, n_ref=None):
    """tree == brute force == the definition on the device's AABBs, both categories."""
    results = {cat: (w.query_aabb(q, cat), w.query_aabb(q, cat, brute_force=True)) for cat in CATS}
    if aabb is None:
        aabb = w.get_derived()[0]
    masks = _masks(kind, shape, removed)
    n_ref = len(q) if n_ref is None else n_ref
    for cat in CATS:
        tree, brute = results[cat]
        _same(tree, brute, (what, cat, "tree vs brute force"))
        off, ids = query_ref.query(aabb[masks[cat]], q[:n_ref], ids=np.flatnonzero(masks[cat]))
        assert np.array_equal(tree[0][:n_ref + 1], off), (what, cat, "offsets vs definition")
        assert np.array_equal(tree[1][:off[-1]], ids), (what, cat, "ids vs definition")
    return results


def _bodies_aabb(w, shape):
    aabb = w.get_derived()[0]
    return aabb[(np.asarray(shape) != scenes.SHAPE_NONE) & (np.asarray(shape) != scenes.SHAPE_PLANE)]


@pytest.fixture(scope="module")
def fixture_world():
    s = mr.scene()
    w = edyn_amd.World(edyn_amd.init_config(gravity=(0.0, 0.0, 0.0)))
    w.set_scene(s)
    w.step_simulation(1)
    return s, w


@pytest.mark.parametrize("which", mq.SETS)
def test_fixture_scene_equals_the_reference_tree(fixture_world, which):
    s, w = fixture_world
    fx = np.load(os.path.join(os.path.dirname(mq.__file__), f"query_aabb_{which}.npz"))
    aabb = w.get_derived()[0]
    assert np.array_equal(aabb, fx["aabb"])   # the device's AABBs are the real engine's
    q = mq.queries(which, s, fx["aabb"])
    assert str(fx["scene_sha256"]) == mr.scene_digest(s) and str(fx["queries_sha256"]) == mr.digest(q)
    for cat in mq.CATEGORIES:
        for brute in (False, True):
            off, ids = w.query_aabb(q, cat, brute_force=brute)
            assert np.array_equal(off, fx[cat + "_offsets"]) and np.array_equal(ids, fx[cat + "_ids"]), (which, cat, brute)


SCENES = {"pile32k": (scenes.headline_pile, 300), "mixed32k": (lambda: scenes.box_pile(32, 32, 32, mixed=True), 120),
          "polyheap32k": (lambda: scenes.polyhedron_heap(32, 32, 32), 60)}


@pytest.mark.parametrize("name", list(SCENES))
def test_tree_equals_brute_force_equals_definition(name):
    gen, steps = SCENES[name]
    scene = gen()
    w = _world(scene)
    w.step_simulation(steps)
    q = _queries(_bodies_aabb(w, scene["shape_type"]), 6000, 17)
    before = w.query_aabb_stats()
    res = _check(w, scene["kind"], scene["shape_type"], q, name)
    after = w.query_aabb_stats()
    # both fill paths of large results ran in this one batch: segments sorted by a wave, and segments packed from the body range
    assert after[0] > before[0] and after[1] > before[1], (before, after)
    counts = np.diff(res["procedural"][0][0].astype(np.int64))
    assert counts[:6].min() == _masks(scene["kind"], scene["shape_type"])["procedural"].sum()   # the huge queries report every body
    assert (counts[6:12] == 0).all() and (counts[12:18] == 0).all()                             # empty and NaN queries nothing
    assert (counts > 32).sum() > 100 and ((counts > 0) & (counts <= 32)).sum() > 100


# Layouts the Morton stage and the Karras build never see in a pile (tests/bplayouts.py): no extent on one, two or all axes, runs of equal
# codes, everyone but an outlier in one cell, a body that contains the scene, and trees of one, two and three leaves (with and without
# static bodies, the other category's tree).
LAYOUTS = {"coincident200": lambda: bl.coincident(200), "line": bl.line, "clusters": bl.clusters, "outlier-first": lambda: bl.outlier(True),
           "outlier-last": lambda: bl.outlier(False), "giant-first": lambda: bl.giant("first"), "giant-static": lambda: bl.giant("static"),
           "counts1": lambda: bl.counts(1, 1), "counts2": lambda: bl.counts(2), "counts3": lambda: bl.counts(3, 4), "counts257": lambda: bl.counts(257, 5)}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_tree_equals_brute_force_equals_definition_on_degenerate_layouts(name):
    """5 000 query boxes of _queries' mix, drawn about the bulk of the scene (the bodies within its 2nd to 98th percentile, so that an
    outlier does not dilute them; the huge, touching and twin queries still reach every body): tree == brute force == definition."""
    scene = LAYOUTS[name]()
    w = _world(scene)
    w.refresh_derived()
    aabb = w.get_derived()[0]
    lo, hi = np.percentile(aabb[:, :3], 2, axis=0), np.percentile(aabb[:, 3:], 98, axis=0)
    bulk = np.all((aabb[:, :3] >= lo - 1) & (aabb[:, 3:] <= hi + 1), axis=1)
    q = _queries(aabb[bulk], 5000 - 12, 17)
    ends = np.concatenate([aabb[:6], aabb[-6:]])   # the first and the last bodies' own boxes, wherever they are
    q = np.concatenate([q, ends]).astype(np.float32)
    res = _check(w, scene["kind"], scene["shape_type"], q, name)
    counts = np.diff(res["procedural"][0][0].astype(np.int64))
    nproc = int(_masks(scene["kind"], scene["shape_type"])["procedural"].sum())
    assert counts[:6].min() == nproc   # the huge queries report every body, the one at 1e6 and the one of radius 500 included
    assert (counts[6:12] == 0).all() and (counts[12:18] == 0).all()


def test_sleepers_removed_added_moved_bodies():
    scene = scenes.box_pile(8, 8, 8, mixed=True)
    n0 = len(scene["kind"])
    w = _world(scene, sleeping=True, max_bodies=n0 + 8)
    w.step_simulation(30)
    w.set_asleep(np.ones(w.n, bool))
    asleep = w.get_asleep()
    assert asleep[1:].any()
    kind, shape = scene["kind"].copy(), scene["shape_type"].copy()
    q = _queries(_bodies_aabb(w, shape), 3000, 5)
    res = _check(w, kind, shape, q, "asleep")
    reported = np.unique(res["procedural"][0][1])
    assert asleep[reported].any()                       # sleeping bodies are reported
    victims = [int(reported[0]), int(reported[len(reported) // 2])]
    w.remove_bodies(victims)
    res = _check(w, kind, shape, q, "removed", removed=victims, aabb=w.get_derived()[0])
    for cat in CATS:
        assert not np.isin(victims, res[cat][0][1]).any()   # never reported
    extra = scenes._empty(2)
    extra["pos"][:] = [(0.0, 40.0, 0.0), (3.0, 40.0, 0.0)]
    extra["shape_type"][:] = scenes.SHAPE_BOX
    extra["shape_param"][:, :3] = 0.5
    extra["kind"][1] = scenes.KIND_STATIC
    w.add_scene(extra)
    kind, shape = np.concatenate([kind, extra["kind"]]), np.concatenate([shape, extra["shape_type"]])
    near = np.float32([[-1, 39, -1, 4, 41, 1]])
    assert np.array_equal(w.query_aabb(near, "procedural")[1], [n0]) and np.array_equal(w.query_aabb(near, "non_procedural")[1], [n0 + 1])
    w.step_simulation(1)
    _check(w, kind, shape, q, "added", removed=victims)
    # set_state WITHOUT a step: the boxes follow the new transforms
    pos, orn, lv, av = w.get_state()
    pos = pos.copy(); pos[1:n0] += np.float32([2.5, 7.0, -1.25])
    orn = orn.copy(); orn[1:n0] = orn[1:n0][::-1]
    w.set_state(pos, orn, lv, av)
    got = {cat: (w.query_aabb(q, cat), w.query_aabb(q, cat, brute_force=True)) for cat in CATS}
    moved = w.query_aabb(np.float32([[-1, 39, -1, 4, 41, 1]]) + np.float32([2.5, 7, -1.25, 2.5, 7, -1.25]), "procedural")
    assert n0 not in moved[1]                           # (appended bodies were not moved)
    w.refresh_derived()
    aabb = w.get_derived()[0]
    masks = _masks(kind, shape, victims)
    for cat in CATS:
        _same(got[cat][0], got[cat][1], ("set_state", cat))
        _same(got[cat][0], query_ref.query(aabb[masks[cat]], q, ids=np.flatnonzero(masks[cat])), ("set_state", cat, "definition"))
    # set_center_of_mass
    w.move_center_of_mass(5, (0.1, -0.05, 0.02))
    w.step_simulation(1)
    _check(w, kind, shape, q, "centre of mass", removed=victims)


def _island_boxes(w):
    L, num = w._L, C.c_uint32(0)
    w._check(L.edynhip_get_island_boxes(w._h, None, None, 0, C.byref(num)))
    labels, boxes = np.zeros(num.value, np.uint32), np.zeros((num.value, 6), np.float32)
    w._check(L.edynhip_get_island_boxes(w._h, labels.ctypes.data, boxes.ctypes.data, num.value, C.byref(num)))
    order = np.argsort(labels)
    return labels[order], boxes[order]


@pytest.mark.parametrize("name", ["islands", "pile"])
def test_island_queries(name):
    scene = scenes.mini_piles(16, 16) if name == "islands" else scenes.box_pile(8, 8, 8)
    w = _world(scene)
    w.step_simulation(20)
    labels, boxes = _island_boxes(w)
    assert len(labels) == (256 if name == "islands" else 1)
    q = _queries(boxes, 4000, 23)
    ref = query_ref.query(boxes, q, ids=labels)
    _same(w.query_aabb(q, "islands"), ref, name)
    _same(w.query_aabb(q, "islands", brute_force=True), ref, name + " brute force")
    assert ref[0][-1] > 1000 and np.isin(ref[1], w.get_derived()[2]).all()


def test_capacity_protocol_and_bad_arguments():
    scene = scenes.box_pile(8, 8, 8)
    w = _world(scene)
    w.step_simulation(10)
    L, h = w._L, w._h
    q = _queries(_bodies_aabb(w, scene["shape_type"]), 500, 3)
    want_off, want_ids = w.query_aabb(q, "procedural", brute_force=True)
    total = C.c_uint32(0)
    off = np.zeros(len(q) + 1, np.uint32)
    assert L.edynhip_query_aabb(h, 0, len(q), q.ctypes.data, 0, off.ctypes.data, None, 0, C.byref(total)) == 0   # ids = NULL counts
    assert total.value == want_off[-1] and np.array_equal(off, want_off)
    GUARD = 0xDEADBEEF
    for cap in (1, total.value // 2, total.value - 1):
        ids = np.full(cap + 64, GUARD, np.uint32)
        off[:] = 0; total.value = 0
        assert L.edynhip_query_aabb(h, 0, len(q), q.ctypes.data, 0, off.ctypes.data, ids.ctypes.data, cap, C.byref(total)) == ERR_CAPACITY
        assert total.value == want_off[-1] and np.array_equal(off, want_off) and (ids[cap:] == GUARD).all()
    ids = np.full(total.value + 64, GUARD, np.uint32)
    assert L.edynhip_query_aabb(h, 0, len(q), q.ctypes.data, 0, off.ctypes.data, ids.ctypes.data, total.value, C.byref(total)) == 0   # the retry
    assert np.array_equal(ids[:total.value], want_ids) and (ids[total.value:] == GUARD).all()
    # n = 0
    off0 = np.full(1, 7, np.uint32); total.value = 9
    assert L.edynhip_query_aabb(h, 1, 0, None, 0, off0.ctypes.data, None, 0, C.byref(total)) == 0 and off0[0] == 0 and total.value == 0
    o, i = w.query_aabb(np.zeros((0, 6), np.float32))
    assert len(o) == 1 and o[0] == 0 and len(i) == 0
    # unknown category / flag bits
    assert L.edynhip_query_aabb(h, 3, len(q), q.ctypes.data, 0, off.ctypes.data, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_query_aabb(h, -1, len(q), q.ctypes.data, 0, off.ctypes.data, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_query_aabb(h, 0, len(q), q.ctypes.data, 2, off.ctypes.data, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_query_aabb_device(h, 0, len(q), q.ctypes.data, 6, off.ctypes.data, None, 0, off.ctypes.data) == ERR_INVALID
    with pytest.raises(EdynHipError):
        w.query_aabb(q, 5)


def test_device_capacity_guard_words(monkeypatch):
    """Overflow on the device entry point, with the switch to the body-range path moved out of the way (EDYNHIP_QUERY_SCAN_RATIO = 1, the
    documented debug knob) so that segments of 33 and more hits take the lane-write + wave-sort path, and a capacity that cuts one of them."""
    import torch
    monkeypatch.setenv("EDYNHIP_QUERY_SCAN_RATIO", "1")
    scene = scenes.box_pile(8, 8, 8)
    w = _world(scene)
    w.step_simulation(10)
    q = _queries(_bodies_aabb(w, scene["shape_type"]), 800, 4)
    before = w.query_aabb_stats()
    want_off, want_ids = w.query_aabb(q, "procedural")
    assert w.query_aabb_stats()[0] > before[0]                # segments were sorted by a wave
    counts = np.diff(want_off.astype(np.int64))
    mid = np.flatnonzero((counts > 32) & (counts <= 4096))
    cut = int(mid[len(mid) // 2])                             # a wave-sorted segment that the capacity cuts in half
    cap = int(want_off[cut]) + int(counts[cut]) // 2
    assert want_off[cut] < cap < want_off[cut + 1] and (counts[cut + 1:] > 32).any() and (counts[:cut] > 32).any()
    dev = torch.device("cuda", 0)
    b = torch.zeros((2 * len(q), 4), dtype=torch.float32, device=dev)
    b[:, :3] = torch.from_numpy(q.reshape(-1, 3)).to(dev)
    GUARD = 0x5EADBEE5
    ids = torch.full((cap + 4096,), GUARD, dtype=torch.int32, device=dev)
    off = torch.zeros(len(q) + 1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    w.query_aabb_device(len(q), b.data_ptr(), off.data_ptr(), ids.data_ptr(), cap, total.data_ptr())
    w.synchronize()
    ids_h = ids.cpu().numpy().view(np.uint32)
    assert (ids_h[cap:] == GUARD).all()                      # nothing at or beyond capacity
    assert np.array_equal(off.cpu().numpy().view(np.uint32), want_off) and int(total.cpu().numpy().view(np.uint32)[0]) == want_off[-1]
    end = int(want_off[cut])                                 # every segment that fits whole is complete and ascending
    assert np.array_equal(ids_h[:end], want_ids[:end])
    assert set(ids_h[end:cap].tolist()) <= set(want_ids[end:int(want_off[cut + 1])].tolist())   # the cut one: hits of its own, unsorted


def test_island_queries_after_set_state_without_a_step():
    """The island boxes come from the query's own per-body boxes: right after edynhip_set_state, before any step recomputes the AABBs."""
    scene = scenes.mini_piles(8, 8)
    w = _world(scene)
    w.step_simulation(20)
    labels_before, boxes_before = _island_boxes(w)
    pos, orn, lv, av = w.get_state()
    pos = pos.copy()
    dyn = scene["kind"] == scenes.KIND_DYNAMIC
    pos[dyn] += np.float32([3.5, 11.0, -2.25])
    w.set_state(pos, orn, lv, av)
    q = _queries(boxes_before, 3000, 31)
    q[100:1600] += np.float32([3.5, 11.0, -2.25, 3.5, 11.0, -2.25])   # half of them where the islands now are
    tree, brute = w.query_aabb(q, "islands"), w.query_aabb(q, "islands", brute_force=True)
    w.refresh_derived()
    aabb, _, island = w.get_derived()
    use = dyn & (scene["shape_type"] != scenes.SHAPE_NONE)
    labels = np.unique(island[use])
    boxes = np.stack([np.concatenate([aabb[use & (island == l), :3].min(0), aabb[use & (island == l), 3:].max(0)]) for l in labels]).astype(np.float32)
    assert np.array_equal(labels, labels_before) and not np.array_equal(boxes, boxes_before)
    ref = query_ref.query(boxes, q, ids=labels)
    _same(tree, ref, "islands after set_state")
    _same(brute, ref, "islands after set_state, brute force")
    assert ref[0][-1] > 1000 and not np.array_equal(ref[0], query_ref.query(boxes_before, q, ids=labels_before)[0])


def test_shard_context_is_rejected():
    from edyn_amd.multi import MultiWorld
    mw = MultiWorld(edyn_amd.init_config(), devices=(0, 0))
    mw.set_scene(scenes.mini_piles(2, 2))
    mw.step_simulation(1)
    ctx = mw._L.edynhip_world_context(mw._h, 0)
    assert ctx
    box = np.float32([[-1, -1, -1, 1, 1, 1]])
    off = np.zeros(2, np.uint32)
    total = C.c_uint32(0)
    assert mw._L.edynhip_query_aabb(ctx, 0, 1, box.ctypes.data, 0, off.ctypes.data, None, 0, C.byref(total)) == ERR_UNSUPPORTED
    assert mw._L.edynhip_query_aabb_device(ctx, 0, 1, box.ctypes.data, 0, off.ctypes.data, None, 0, off.ctypes.data) == ERR_UNSUPPORTED
    mw.close()


def test_device_entry_equals_host_and_needs_no_synchronisation():
    import torch
    scene = scenes.box_pile(8, 8, 8, mixed=True)
    a, b = _world(scene), _world(scene)
    a.step_simulation(20); b.step_simulation(20)
    q = _queries(_bodies_aabb(a, scene["shape_type"]), 20000, 9)
    dev = torch.device("cuda", 0)
    boxes = torch.zeros((2 * len(q), 4), dtype=torch.float32, device=dev)
    boxes[:, :3] = torch.from_numpy(q.reshape(-1, 3)).to(dev)
    for cat in ("procedural", "non_procedural", "islands"):
        host = a.query_aabb(q, cat)
        off = torch.zeros(len(q) + 1, dtype=torch.int32, device=dev)
        ids = torch.zeros(max(1, len(host[1])), dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        a.query_aabb_device(len(q), boxes.data_ptr(), off.data_ptr(), ids.data_ptr(), len(host[1]), total.data_ptr(), category=cat)
        a.step_simulation(1); b.step_simulation(1)   # enqueued behind the query on the same stream, no synchronisation in between
        a.synchronize()
        assert int(total.cpu().numpy().view(np.uint32)[0]) == host[0][-1]
        _same((off.cpu().numpy().view(np.uint32), ids.cpu().numpy().view(np.uint32)[:len(host[1])]), host, ("device", cat))
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)


def _snapshot(w):
    return w.get_state(), w.get_pairs(), w.get_manifolds()


def test_queries_do_not_perturb_steps_or_raycasts():
    scene = scenes.box_pile(16, 16, 16)
    a, b = _world(scene), _world(scene)
    a.step_simulation(30); b.step_simulation(30)
    q = _queries(_bodies_aabb(a, scene["shape_type"]), 4000, 6)
    rng = np.random.default_rng(2)
    p0 = rng.uniform(-10, 10, (20000, 3)).astype(np.float32)
    p1 = (p0 + rng.normal(size=(20000, 3)) * 8).astype(np.float32)
    for step in range(50):
        if step % 5 == 0:   # rays and boxes interleaved on the shared tree
            r0 = a.raycast(p0, p1)
            for cat in ("procedural", "non_procedural", "islands"):
                a.query_aabb(q, cat)
            r1 = a.raycast(p0, p1)
            assert r0.tobytes() == r1.tobytes()
            assert a.raycast(p0, p1).tobytes() == b.raycast(p0, p1).tobytes()
        else:
            a.query_aabb(q[:200], ("procedural", "non_procedural", "islands")[step % 3])
        a.step_simulation(1); b.step_simulation(1)
    sa, sb = _snapshot(a), _snapshot(b)
    for x, y in zip(sa[0], sb[0]):
        assert np.array_equal(x, y)
    assert np.array_equal(sa[1], sb[1]) and np.array_equal(sa[2], sb[2])
