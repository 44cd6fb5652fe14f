"""Raycast queries on the device (edynhip_raycast / World.raycast): edyn::raycast's definition, the query tree against the
brute-force walk over every body, the reference's own shape_raycast on the device's state, and that a raycast changes nothing a
later step computes."""
import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes

import bplayouts as bl
import raycast_ref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FLT_MAX = np.float32(np.finfo(np.float32).max)


def _world(scene, sleeping=False, max_bodies=0):
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, sleeping=sleeping,
                                            max_bodies=max_bodies))
    w.set_scene(scene)
    return w


def _one_box(pos=(0.5, 0.5, 0.5), kind=scenes.KIND_STATIC):
    s = scenes._empty(1)
    s["kind"][0] = kind
    s["pos"][0] = pos
    s["shape_type"][0] = scenes.SHAPE_BOX
    s["shape_param"][0, :3] = 0.5
    return s


def _shapes_scene():
    """Every shape the device steps: boxes, spheres, capsules and cylinders on all three axes, a plane, centre-of-mass offsets,
    static and dynamic bodies, and one amorphous body - on a grid, nothing overlapping."""
    kinds = [(scenes.SHAPE_BOX, (0.5, 0.3, 0.4, 0)), (scenes.SHAPE_SPHERE, (0.45, 0, 0, 0))]
    kinds += [(scenes.SHAPE_CAPSULE, (0.25, 0.4, a, 0)) for a in range(3)] + [(scenes.SHAPE_CYLINDER, (0.3, 0.35, a, 0)) for a in range(3)]
    g = 6
    n = 1 + g * g * 2
    s = scenes._empty(n)
    scenes._add_plane(s)
    rng = np.random.default_rng(5)
    i = 1
    for y in range(2):
        for x in range(g):
            for z in range(g):
                st, sp = kinds[(i - 1) % len(kinds)]
                s["shape_type"][i] = st
                s["shape_param"][i] = sp
                s["pos"][i] = (x * 2.0 - g, 1.0 + 2.0 * y, z * 2.0 - g)
                q = rng.normal(size=4)
                s["orn"][i] = (q / np.linalg.norm(q)).astype(np.float32)
                s["kind"][i] = scenes.KIND_STATIC if (i % 3 == 0) else scenes.KIND_DYNAMIC
                i += 1
    s["shape_type"][n - 1] = 0   # amorphous: never a candidate
    s["com"] = np.zeros((n, 3), np.float32)
    s["com"][5] = (0.1, -0.05, 0.02)
    s["com"][9] = (-0.08, 0.1, 0.0)
    return s


def _random_rays(n, lo, hi, seed, min_len=0.5, max_len=50.0):
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = rng.uniform(min_len, max_len, size=(n, 1))
    return p0, (p0 + d * ln).astype(np.float32)


def _grazing_rays(aabb, n, seed):
    """Rays along the faces of the candidate boxes (AABB grown by 0.1): exactly on the face plane, and one ulp either side."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, len(aabb), n)
    mn = aabb[b, :3] - np.float32(0.1)
    mx = aabb[b, 3:] + np.float32(0.1)
    axis = rng.integers(0, 3, n)
    t = rng.uniform(-0.2, 1.2, size=(n, 3)).astype(np.float32)
    p0 = (mn + (mx - mn) * t).astype(np.float32)
    side = rng.integers(0, 2, n).astype(bool)
    face = np.where(side, mx[np.arange(n), axis], mn[np.arange(n), axis])
    nudge = rng.integers(-1, 2, n)
    face = np.where(nudge > 0, np.nextafter(face, np.float32(np.inf)), np.where(nudge < 0, np.nextafter(face, np.float32(-np.inf)), face))
    p0[np.arange(n), axis] = face
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[np.arange(n), axis] = 0
    p1 = (p0 + d * np.float32(3)).astype(np.float32)
    return p0, p1


def _assert_same(a, b, what):
    for f in ("body", "fraction", "normal", "feature", "feature_index"):
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f, int(np.sum(a[f] != b[f]) if a[f].ndim == 1 else np.sum(np.any(a[f] != b[f], axis=1))))


def test_reference_raycast_box():
    """test/edyn/collision/test_raycast.cpp, transcribed."""
    w = _world(_one_box())
    w.step_simulation(1)
    r = w.raycast((2, 2, 2), (0, 0, 0))
    assert r["body"][0] == 0 and r["fraction"][0] == np.float32(0.5) and r["feature"][0] == _capi.RAYCAST_BOX_FACE
    r = w.raycast((0.5, 2, 0.5), (0.5, 0, 0.5))
    assert r["body"][0] == 0 and r["fraction"][0] == np.float32(0.5)
    assert r["feature"][0] == _capi.RAYCAST_BOX_FACE and r["feature_index"][0] == 2
    assert np.array_equal(r["normal"][0], np.float32([0, 1, 0]))


def test_miss_empty_single_ignore_chunks():
    w = _world(scenes.box_pile(4, 4, 4))
    w.step_simulation(5)
    r = w.raycast((100, 100, 100), (101, 100, 100))
    assert r["body"][0] == NONE and r["fraction"][0] == FLT_MAX and r["feature"][0] == 0
    assert len(w.raycast(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    down = w.raycast((0, 20, 0), (0, -1, 0))   # onto the pile from above
    top = down["body"][0]
    assert top not in (NONE, 0) and 0 < down["fraction"][0] < 1
    again = w.raycast((0, 20, 0), (0, -1, 0), ignore=[top])
    assert again["body"][0] not in (NONE, top) and again["fraction"][0] > down["fraction"][0]
    every = w.raycast((0, 20, 0), (0, -1, 0), ignore=np.arange(1, w.n))
    assert every["body"][0] == 0   # the plane
    p0, p1 = _random_rays(1 << 20, -8, 8, 11)
    one = w.raycast(p0, p1)
    four = w.raycast(np.tile(p0, (4, 1)), np.tile(p1, (4, 1)))   # 4M rays: four internal chunks
    _assert_same(four, np.tile(one, 4), "4M rays")
    _assert_same(w.raycast(p0[:1000], p1[:1000], brute_force=True), one[:1000], "brute force")


def test_sleeping_hit_amorphous_and_removed_never():
    s = _shapes_scene()
    w = _world(s, sleeping=True)
    w.step_simulation(2)
    asleep = np.ones(w.n, bool)
    w.set_asleep(asleep)
    assert w.get_asleep()[1:-1].any()
    aabb, _, _ = w.get_derived()
    p0, p1 = _random_rays(200000, -8, 8, 3)
    r = w.raycast(p0, p1)
    hit = set(np.unique(r["body"]).tolist())
    assert (w.n - 1) not in hit                        # amorphous
    assert len(hit - {NONE}) > 0.5 * (w.n - 1)         # sleeping bodies included
    victim = int(np.bincount(r["body"][r["body"] != NONE]).argmax())
    w.remove_bodies([victim])
    r2 = w.raycast(p0, p1)
    assert victim not in set(np.unique(r2["body"]).tolist())
    _assert_same(r2, w.raycast(p0, p1, brute_force=True), "after removal")


SCENES = {"pile32k": (scenes.headline_pile, 300), "mixed32k": (lambda: scenes.box_pile(32, 32, 32, mixed=True), 120),
          "polyheap32k": (lambda: scenes.polyhedron_heap(32, 32, 32), 60), "islands256k": (scenes.c4_islands, 20)}


@pytest.mark.parametrize("name", list(SCENES))
def test_tree_equals_brute_force(name):
    gen, steps = SCENES[name]
    scene = gen()
    w = _world(scene)
    w.step_simulation(steps)
    aabb, _, _ = w.get_derived()
    shaped = scene["shape_type"] != scenes.SHAPE_PLANE
    lo, hi = aabb[shaped, :3].min(0), aabb[shaped, 3:].max(0)
    n = 1 << 20
    p0, p1 = _random_rays(n - n // 4, lo - 2, hi + 2, 7)
    g0, g1 = _grazing_rays(aabb[shaped], n // 4, 8)
    p0, p1 = np.concatenate([p0, g0]), np.concatenate([p1, g1])
    tree = w.raycast(p0, p1)
    brute = w.raycast(p0, p1, brute_force=True)
    _assert_same(tree, brute, name)
    assert (tree["body"] != NONE).mean() > 0.2


# Layouts the Morton stage and the Karras build never see in a pile (tests/bplayouts.py): no extent on one, two or all axes, runs of equal
# codes, everyone but an outlier in one cell, a body that contains the scene, and trees of one, two and three leaves.
LAYOUTS = {"coincident200": lambda: bl.coincident(200), "line": bl.line, "clusters": bl.clusters, "outlier-first": lambda: bl.outlier(True),
           "outlier-last": lambda: bl.outlier(False), "giant-first": lambda: bl.giant("first"), "giant-static": lambda: bl.giant("static"),
           "counts1": lambda: bl.counts(1), "counts2": lambda: bl.counts(2), "counts3": lambda: bl.counts(3), "counts257": lambda: bl.counts(257, 4)}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_tree_equals_brute_force_on_degenerate_layouts(name):
    """15 000 random rays about the bulk of the scene (its 2nd to 98th percentile, so that an outlier does not dilute them), 5 000 along
    the faces of the candidate boxes, and 100 aimed at the centres of the first and the last body from afar: tree == brute force."""
    scene = LAYOUTS[name]()
    w = _world(scene)
    w.refresh_derived()
    aabb, _, _ = w.get_derived()
    lo, hi = np.percentile(aabb[:, :3], 2, axis=0), np.percentile(aabb[:, 3:], 98, axis=0)
    p0, p1 = _random_rays(15000, lo - 2, hi + 2, 7)
    g0, g1 = _grazing_rays(aabb, 5000, 8)
    a0, _ = _random_rays(100, lo - 2, hi + 2, 9)
    ends = scene["pos"][np.where(np.arange(100) & 1, len(aabb) - 1, 0)]
    a1 = (ends + (ends - a0) * np.float32(0.01)).astype(np.float32)   # a little beyond the centre
    p0, p1 = np.concatenate([p0, g0, a0]), np.concatenate([p1, g1, a1])
    tree = w.raycast(p0, p1)
    brute = w.raycast(p0, p1, brute_force=True)
    _assert_same(tree, brute, name)
    assert (tree["body"] != NONE).any()


def _reference_best(ref, scene, pos, orn, aabb, com, p0, p1):
    """edyn::raycast over every body with the reference's intersect_segment_aabb and shape_raycast, on the device's state."""
    origin = pos.copy()
    best = (FLT_MAX, NONE, None)
    fmin = (aabb[:, :3] - np.float32(0.1)).astype(np.float32)
    fmax = (aabb[:, 3:] + np.float32(0.1)).astype(np.float32)
    smin, smax = np.minimum(p0, p1), np.maximum(p0, p1)
    # a superset of the candidates: the rounded test accepts segments up to a few ulps of the box's coordinates outside it (the
    # planes' half-space boxes reach 1e5, where an ulp is 0.008)
    m = (1e-3 + 1e-5 * np.maximum(np.abs(fmin), np.abs(fmax)).max(axis=1))[:, None]
    near = np.all((fmin <= smax + m) & (fmax >= smin - m), axis=1)
    for b in np.flatnonzero(near):
        st = int(scene["shape_type"][b])
        if st == 0 or not ref.intersect_segment_aabb(p0, p1, fmin[b], fmax[b]):
            continue
        res = ref.shape_raycast(st, scene["shape_param"][b], origin[b] if com is None else com[b], orn[b], p0, p1)
        if res[0] < best[0]:
            best = (res[0], b, res)
    return best


@pytest.mark.skipif(not raycast_ref.available(), reason="oracle/_ref/libedynref.so is absent (built where the reference sources are)")
@pytest.mark.parametrize("case", ["shapes", "pile"])
def test_matches_reference_shape_raycast_on_device_state(case):
    ref = raycast_ref.RefRaycast()
    scene = _shapes_scene() if case == "shapes" else scenes.box_pile(8, 8, 8)
    w = _world(scene)
    w.step_simulation(40)
    pos, orn, _, _ = w.get_state()
    aabb, _, _ = w.get_derived()
    com = None
    if "com" in scene:   # shapes sit at origin = to_world(-com, pos, orn) (raycast.cpp:31-34)
        q = orn[:, :3].astype(np.float32); qw = orn[:, 3:4].astype(np.float32)
        v = -scene["com"].astype(np.float32)
        t = np.cross(q, v) + qw * v
        com = np.where(np.any(scene["com"] != 0, axis=1)[:, None], pos + (v + 2 * np.cross(q, t)), pos).astype(np.float32)
    shaped = scene["shape_type"] > 0
    lo, hi = aabb[shaped & (scene["shape_type"] != scenes.SHAPE_PLANE), :3].min(0), aabb[shaped & (scene["shape_type"] != scenes.SHAPE_PLANE), 3:].max(0)
    p0, p1 = _random_rays(2000, lo - 1, hi + 1, 21, max_len=20.0)
    dev = w.raycast(p0, p1)
    checked = 0
    for i in range(len(p0)):
        f, b, res = _reference_best(ref, scene, pos, orn, aabb, com, p0[i], p1[i])
        assert dev["body"][i] == b, (i, dev[i], b, f)
        if b == NONE:
            continue
        assert dev["fraction"][i] == res[0], (i, dev[i], res)
        assert np.array_equal(dev["normal"][i], res[1]), (i, dev[i], res)
        assert dev["feature"][i] == res[2] and dev["feature_index"][i] == res[3], (i, dev[i], res)
        checked += 1
    assert checked > 200


def _snapshot(w):
    return w.get_state(), w.get_pairs(), w.get_manifolds()


def _assert_snap_equal(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2])


def test_raycast_does_not_perturb_steps():
    scene = scenes.box_pile(16, 16, 16)
    a, b = _world(scene, max_bodies=len(scene["kind"]) + 8), _world(scene, max_bodies=len(scene["kind"]) + 8)
    a.step_simulation(40); b.step_simulation(40)
    p0, p1 = _random_rays(1 << 18, -10, 10, 4)
    a.raycast(p0, p1)
    a.raycast(p0, p1, ignore=[1, 2, 3])
    a.step_simulation(30); b.step_simulation(30)
    _assert_snap_equal(_snapshot(a), _snapshot(b))
    # edits between the steps: the raycast sees them, and still leaves the steps alone
    pos, orn, lv, av = a.get_state()
    pos = pos.copy(); pos[1] += np.float32([0, 30, 0])
    a.set_state(pos, orn, lv, av); b.set_state(pos, orn, lv, av)
    r = a.raycast(pos[1] + np.float32([0, 5, 0]), pos[1] - np.float32([0, 5, 0]))
    assert r["body"][0] == 1 and abs(r["fraction"][0] - 0.45) < 2e-3
    extra = _one_box(pos=(0.0, 60.0, 0.0), kind=scenes.KIND_DYNAMIC)
    a.add_scene(extra); b.add_scene(extra)
    r = a.raycast((0, 70, 0), (0, 50, 0))
    assert r["body"][0] == a.n - 1 and abs(r["fraction"][0] - 0.475) < 1e-5
    a.raycast(p0, p1)
    a.step_simulation(20); b.step_simulation(20)
    _assert_snap_equal(_snapshot(a), _snapshot(b))


def test_raycast_device_equals_host():
    import torch
    w = _world(scenes.box_pile(8, 8, 8, mixed=True))
    w.step_simulation(20)
    p0, p1 = _random_rays(100000, -6, 6, 9)
    host = w.raycast(p0, p1, ignore=[5, 6])
    dev = torch.device("cuda", 0)
    t0 = torch.zeros((len(p0), 4), dtype=torch.float32, device=dev); t0[:, :3] = torch.from_numpy(p0).to(dev)
    t1 = torch.zeros((len(p0), 4), dtype=torch.float32, device=dev); t1[:, :3] = torch.from_numpy(p1).to(dev)
    out = torch.zeros((len(p0), 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    w.raycast_device(len(p0), t0.data_ptr(), t1.data_ptr(), out.data_ptr(), ignore=[5, 6])
    w.synchronize()
    got = out.cpu().numpy().view(_capi.RAYCAST_HIT_DTYPE).reshape(-1)
    _assert_same(got, host, "device pointers")
