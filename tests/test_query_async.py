"""Queries as tickets (edynhip_raycast_submit / edynhip_query_aabb_submit / edynhip_query_poll / edynhip_*_collect /
edynhip_query_release; World.raycast_submit ... World.query_release): a ticket answers what the synchronous entry points answer for
the state at its submit - rays byte for byte, per-ray ignore lists included, box lists per category, and the of-interest list against
its definition on edynhip_get_derived's island labels - whatever is enqueued, asked synchronously, removed or collected in between."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd._capi import EdynHipError

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_query_aabb as mq   # noqa: E402
import make_raycast as mr      # noqa: E402
from test_raycast_golden import _same as same_as_reference   # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ERR_INVALID, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -4, -6
CATS = ("procedural", "non_procedural", "islands")


@pytest.fixture(scope="module")
def ray_world():
    s = mr.scene()
    w = edyn_amd.World(edyn_amd.init_config(gravity=(0.0, 0.0, 0.0)))
    w.set_scene(s)
    w.step_simulation(1)
    assert w.n == 148
    p0, p1 = mr.rays("random", s)
    return s, w, p0, p1


def _collect(w, t):
    out = w.query_collect(t)
    assert w.query_poll(t)   # a collected ticket is done
    w.query_release(t)
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_rays_equal_the_synchronous_call(ray_world, n):
    s, w, p0, p1 = ray_world
    a, b = p0[1000:1000 + n], p1[1000:1000 + n]
    got = _collect(w, w.raycast_submit(a, b))
    assert got.dtype == _capi.RAYCAST_HIT_DTYPE and len(got) == n
    assert got.tobytes() == w.raycast(a, b).tobytes()
    brute = _collect(w, w.raycast_submit(a, b, brute_force=True))
    assert brute.tobytes() == w.raycast(a, b, brute_force=True).tobytes()


def test_golden_rays_through_one_ticket(ray_world):
    s, w, p0, p1 = ray_world
    fx = np.load(os.path.join(os.path.dirname(mr.__file__), "raycast_random.npz"))
    assert str(fx["rays_sha256"]) == mr.digest(p0, p1) and str(fx["scene_sha256"]) == mr.scene_digest(s)
    ref = fx["result"]
    dev = _collect(w, w.raycast_submit(p0, p1))
    assert len(dev) == 20000
    ok = same_as_reference(dev, ref)
    bad = np.flatnonzero(~ok)
    ties = 0
    for i in bad:   # an exact tie: with the device's choice ignored, the reference's body comes out
        if dev["fraction"][i] != ref["fraction"][i] or dev["body"][i] == NONE:
            continue
        again = _collect(w, w.raycast_submit(p0[i:i + 1], p1[i:i + 1], ignore=[[int(dev["body"][i])]]))
        if same_as_reference(again, ref[i:i + 1])[0]:
            ties += 1
    assert ties == len(bad), (len(bad) - ties, [(int(i), dev[i], ref[i]) for i in bad[:5]])
    assert (ref["entity"] != NONE).sum() > 2000


def test_per_ray_ignore_lists(ray_world):
    s, w, p0, p1 = ray_world
    plain = w.raycast(p0[:4000], p1[:4000])
    rays = np.flatnonzero(plain["body"] != NONE)[:256]   # rays that hit something: ignoring it changes the answer
    assert len(rays) == 256
    a, b = p0[rays], p1[rays]
    first = plain["body"][rays]
    rng = np.random.default_rng(5)
    lists = []
    for k in range(256):
        f = int(first[k])
        kind = k % 4
        if kind == 0:
            lists.append([])
        elif kind == 1:
            lists.append([f])
        elif kind == 2:
            nxt = int(w.raycast(a[k], b[k], ignore=[f])["body"][0])
            lists.append([f] + ([nxt] if nxt != NONE else []))
        else:   # 33 entries: duplicates, an index beyond the bodies, the hit body somewhere among them
            l = list(rng.integers(0, w.n, 30)) + [f, f, w.n + int(rng.integers(0, 1000))]
            lists.append([int(x) for x in rng.permutation(l)])
            assert len(lists[-1]) == 33
    got = _collect(w, w.raycast_submit(a, b, ignore=lists))
    changed = 0
    for k in range(256):
        own = w.raycast(a[k], b[k], ignore=lists[k])
        assert got[k:k + 1].tobytes() == own.tobytes(), (k, lists[k], got[k], own[0])
        changed += int(got["body"][k] != first[k])
    assert changed >= 150   # three lists in four name the body the plain ray hits
    # the same lists laid end to end, with offsets that do not start at 0
    ids = np.concatenate([np.uint32([9, 9, 9])] + [np.asarray(l, np.uint32) for l in lists])
    off = np.uint32(3) + np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
    assert _collect(w, w.raycast_submit(a, b, ignore=ids, ignore_offsets=off)).tobytes() == got.tobytes()


def _moved(w):
    pos, orn, lv, av = w.get_state()
    pos = pos.copy()
    pos[:, 0] += 0.75
    pos[:, 1] += 0.25
    return pos, orn, lv, av


def test_stream_order_and_synchronous_calls_in_between(ray_world):
    s, w, p0, p1 = ray_world
    a, b = p0[:500], p1[:500]
    aabb = w.get_derived()[0]
    q = mq.queries("bodies", s, aabb, 200)
    state0 = w.get_state()
    before = w.raycast(a, b)
    before_q = {c: w.query_aabb(q, c) for c in CATS[:2]}
    cap = int(before_q["procedural"][0][-1] + before_q["non_procedural"][0][-1]) + 4096
    ta = w.raycast_submit(a, b)
    tqa = w.query_aabb_submit(q, 3, cap)
    w.set_state(*_moved(w))
    tb = w.raycast_submit(a, b)
    tqb = w.query_aabb_submit(q, 3, cap)
    # synchronous calls between submit and collect: right themselves, and they change no ticket
    after = w.raycast(a, b, ignore=[1, 2, 3])
    after_plain = w.raycast(a, b)
    after_q = {c: w.query_aabb(q, c) for c in CATS[:2]}
    w.query_aabb(q[:7] + np.float32(0.5), "non_procedural")   # (other boxes: the synchronous path's buffers hold them now)
    gb = w.query_collect(tb)   # B first
    ga = w.query_collect(ta)
    qb = w.query_collect(tqb)
    qa = w.query_collect(tqa)
    for t in (ta, tb, tqa, tqb):
        w.query_release(t)
    assert not np.array_equal(before, after_plain)   # the move shows
    assert after.tobytes() == w.raycast(a, b, ignore=[1, 2, 3], brute_force=True).tobytes()
    for c in CATS[:2]:
        brute = w.query_aabb(q, c, brute_force=True)
        assert np.array_equal(after_q[c][0], brute[0]) and np.array_equal(after_q[c][1], brute[1])
    assert ga.tobytes() == before.tobytes() and gb.tobytes() == after_plain.tobytes()
    for got, ref in ((qa, before_q), (qb, after_q)):
        for k, c in enumerate(CATS[:2]):
            off, ids = ref[c]
            for i in range(len(q)):
                assert np.array_equal(got[1][got[0][4 * i + k]:got[0][4 * i + k + 1]], ids[off[i]:off[i + 1]]), (c, i)
    w.set_state(*state0)   # (the world is shared with the other tests)
    assert w.raycast(a, b).tobytes() == before.tobytes()
    chk = {c: w.query_aabb(q, c) for c in CATS[:2]}
    for c in CATS[:2]:
        assert np.array_equal(chk[c][0], before_q[c][0]) and np.array_equal(chk[c][1], before_q[c][1])


def test_ticket_limits_and_lifetime():
    s = mr.scene()
    w = edyn_amd.World(edyn_amd.init_config(gravity=(0.0, 0.0, 0.0)))
    w.set_scene(s)
    w.step_simulation(1)
    p0, p1 = mr.rays("random", s, 800)
    ref = w.raycast(p0, p1)
    tickets = [w.raycast_submit(p0[100 * k:100 * k + 100], p1[100 * k:100 * k + 100]) for k in range(8)]
    assert len(set(tickets)) == 8 and 0 not in tickets
    with pytest.raises(EdynHipError) as e:
        w.raycast_submit(p0[:1], p1[:1])
    assert e.value.code == ERR_CAPACITY
    with pytest.raises(EdynHipError) as e:
        w.query_aabb_submit(np.float32([[-1, -1, -1, 1, 1, 1]]), 1, 16)
    assert e.value.code == ERR_CAPACITY
    # bodies removed after the submits: the tickets answer from the state they were submitted on
    hit = np.unique(ref["body"][ref["body"] != NONE])[:20]
    w.remove_bodies([int(x) for x in hit])
    assert not np.array_equal(w.raycast(p0, p1)["body"], ref["body"])
    for k in (3, 0, 7, 1, 2, 6, 5, 4):   # any order
        assert w.query_collect(tickets[k]).tobytes() == ref[100 * k:100 * k + 100].tobytes(), k
    assert w.query_collect(tickets[3]).tobytes() == ref[300:400].tobytes()   # twice
    w.query_release(tickets[2])
    for call in (w.query_collect, w.query_poll, w.query_release):
        with pytest.raises(EdynHipError) as e:
            call(tickets[2])
        assert e.value.code == ERR_INVALID
    with pytest.raises(EdynHipError) as e:
        w.query_poll(123456)
    assert e.value.code == ERR_INVALID
    # a box ticket is no ray ticket, and the slot that came free is the one that is taken, under a new value
    tq = w.query_aabb_submit(np.float32([[-1, -1, -1, 1, 1, 1]]), 1, 64)
    assert tq not in tickets
    hits, n = C.c_void_p(None), C.c_uint32(0)
    assert w._L.edynhip_raycast_collect(w._h, tq, C.byref(hits), C.byref(n)) == ERR_INVALID
    view = _capi.QueryAabbView()
    assert w._L.edynhip_query_aabb_collect(w._h, tickets[0], C.byref(view)) == ERR_INVALID
    assert w.query_collect(tickets[7]).tobytes() == ref[700:800].tobytes()   # the others are as they were
    w.detach()   # seven tickets outstanding, one of them never collected


@pytest.fixture(scope="module")
def box_world():
    s = mr.scene()
    w = edyn_amd.World(edyn_amd.init_config(gravity=(0.0, 0.0, 0.0)))
    w.set_scene(s)
    w.step_simulation(1)
    aabb = w.get_derived()[0]
    every = np.float32([[-1e6] * 3 + [1e6] * 3])   # the first box meets everything: no prefix of the boxes has empty lists only
    q = np.concatenate([every, mq.queries("bodies", s, aabb, 200), mq.queries("planes", s, aabb, 100)]).astype(np.float32)
    ref = {c: w.query_aabb(q, c) for c in CATS}
    assert all(ref[c][0][-1] > 50 and ref[c][0][1] > 0 for c in CATS)
    isl = w.get_derived()[2]
    members = (np.asarray(s["kind"]) == scenes.KIND_DYNAMIC) & (np.asarray(s["shape_type"]) != scenes.SHAPE_NONE)
    return w, q, ref, lambda labels: np.flatnonzero(np.isin(isl, labels) & members)   # the definition of list 3


@pytest.mark.parametrize("n", [0, 1, 64, 65, 300])
def test_boxes_equal_the_synchronous_call(box_world, n):
    w, q, ref, _interest = box_world
    want = (1 + (np.arange(n) + n) % 15).astype(np.uint8)   # masks 1 .. 15, cycled
    total, offsets = 0, np.zeros(1, np.uint32)
    if n:   # a capacity of total - 1: refused, offsets and total come all the same
        probe = w.query_aabb_submit(q[:n], want, 0)
        with pytest.raises(EdynHipError) as e:
            w.query_collect(probe)
        w.query_release(probe)
        total, offsets = e.value.total, e.value.offsets
        assert e.value.code == ERR_CAPACITY and total > 0 and offsets[-1] == total and len(offsets) == 4 * n + 1
        t1 = w.query_aabb_submit(q[:n], want, total - 1)
        with pytest.raises(EdynHipError) as e:
            w.query_collect(t1)
        assert e.value.code == ERR_CAPACITY and e.value.total == total and np.array_equal(e.value.offsets, offsets)
        view = _capi.QueryAabbView()
        assert w._L.edynhip_query_aabb_collect(w._h, t1, C.byref(view)) == ERR_CAPACITY and not view.ids and view.total == total
        w.query_release(t1)
    off, ids = _collect(w, w.query_aabb_submit(q[:n], want, total))   # exactly enough
    assert len(off) == 4 * n + 1 and off[0] == 0 and off[-1] == total == len(ids)
    assert np.array_equal(off, offsets)
    for i in range(n):
        for k, c in enumerate(CATS):
            lst = ids[off[4 * i + k]:off[4 * i + k + 1]]
            r_off, r_ids = ref[c]
            exp = r_ids[r_off[i]:r_off[i + 1]] if want[i] & (1 << k) else r_ids[:0]
            assert np.array_equal(lst, exp), (i, c, int(want[i]))
        lst = ids[off[4 * i + 3]:off[4 * i + 4]]
        r_off, r_ids = ref["islands"]
        exp = _interest(r_ids[r_off[i]:r_off[i + 1]]) if want[i] & 8 else r_ids[:0]
        assert np.array_equal(lst, exp), (i, "of interest", int(want[i]))
    if n:
        brute = _collect(w, w.query_aabb_submit(q[:n], want, total, brute_force=True))
        assert np.array_equal(brute[0], off) and np.array_equal(brute[1], ids)


@pytest.mark.parametrize("sleeping", [False, True])
def test_of_interest_lists_on_islands(sleeping):
    scene = scenes.mini_piles(3, 3)
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, sleeping=sleeping))
    w.set_scene(scene)
    w.step_simulation(30)
    dyn = np.asarray(scene["kind"]) == scenes.KIND_DYNAMIC
    shaped = np.asarray(scene["shape_type"]) != scenes.SHAPE_NONE
    pos = w.get_state()[0]
    rng = np.random.default_rng(11)
    c = pos[rng.integers(1, w.n, 60)]
    h = rng.uniform(0.3, 9.0, (60, 1)).astype(np.float32)
    q = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    q = np.concatenate([q, np.float32([[-1e6] * 3 + [1e6] * 3, [500, 500, 500, 501, 501, 501]])])
    r_off, r_ids = w.query_aabb(q, "islands")
    isl = w.get_derived()[2]
    # not vacuous: some box reports two islands or more, and some island has three members or more
    assert np.diff(r_off.astype(np.int64)).max() >= 2
    assert np.bincount(isl[dyn]).max() >= 3
    want = np.where(np.arange(len(q)) % 3 == 0, 8, 12).astype(np.uint8)   # of interest alone, and with the islands list
    t = w.query_aabb_submit(q, want, 0)
    with pytest.raises(EdynHipError) as e:
        w.query_collect(t)
    w.query_release(t)
    off, ids = _collect(w, w.query_aabb_submit(q, want, e.value.total))
    seen = 0
    for i in range(len(q)):
        labels = r_ids[r_off[i]:r_off[i + 1]]
        exp = np.flatnonzero(np.isin(isl, labels) & dyn & shaped)
        assert np.array_equal(ids[off[4 * i + 3]:off[4 * i + 4]], exp), i
        assert np.array_equal(ids[off[4 * i + 2]:off[4 * i + 3]], labels if want[i] & 4 else labels[:0]), i
        assert off[4 * i] == off[4 * i + 2]   # lists 0 and 1 were not wanted
        seen += len(exp)
    assert seen > 64 * 9   # the everything-box alone lists every pile
    assert len(ids[off[4 * (len(q) - 1) + 3]:off[4 * len(q)]]) == 0   # the far box: nothing


def test_refusals(ray_world):
    s, w, p0, p1 = ray_world
    L, h = w._L, w._h
    t = C.c_uint64(0)
    a, b = np.ascontiguousarray(p0[:3]), np.ascontiguousarray(p1[:3])
    ids = np.uint32([1, 2, 3])
    box = np.float32([[-1, -1, -1, 1, 1, 1]] * 3)
    ok_want = np.uint8([1, 2, 15])

    def rays(off, flags=0, idp=ids.ctypes.data):
        off = np.asarray(off, np.uint32)
        return L.edynhip_raycast_submit(h, 3, a.ctypes.data, b.ctypes.data, off.ctypes.data, idp, flags, C.byref(t))

    assert rays([0, 2, 1, 3]) == ERR_INVALID          # descending offsets
    assert rays([3, 2, 2, 2]) == ERR_INVALID
    assert rays([0, 1, 2, 3], flags=2) == ERR_INVALID  # unknown flag bits
    assert rays([0, 1, 2, 3], idp=None) == ERR_INVALID  # ids named, none given
    assert L.edynhip_query_aabb_submit(h, 3, box.ctypes.data, ok_want.ctypes.data, 64, 2, C.byref(t)) == ERR_INVALID
    for bad in (16, 32, 128, 17):
        wm = np.uint8([1, bad, 2])
        assert L.edynhip_query_aabb_submit(h, 3, box.ctypes.data, wm.ctypes.data, 64, 0, C.byref(t)) == ERR_INVALID
    assert L.edynhip_query_aabb_submit(h, 3, box.ctypes.data, None, 64, 0, C.byref(t)) == ERR_INVALID
    # none of the refused calls took a slot: eight still fit
    got = [w.raycast_submit(a, b) for _ in range(8)]
    for x in got:
        w.query_release(x)
    assert rays([0, 1, 2, 3]) == 0
    w.query_release(t.value)


def test_shard_context_is_refused():
    from edyn_amd.multi import MultiWorld
    mw = MultiWorld(edyn_amd.init_config(), devices=(0, 0))
    mw.set_scene(scenes.mini_piles(2, 2))
    mw.step_simulation(1)
    ctx = mw._L.edynhip_world_context(mw._h, 0)
    assert ctx
    t = C.c_uint64(0)
    p = np.float32([[0, 5, 0], [0, -5, 0]])
    box = np.float32([[-1, -1, -1, 1, 1, 1]])
    want = np.uint8([15])
    assert mw._L.edynhip_raycast_submit(ctx, 1, p[0:1].ctypes.data, p[1:2].ctypes.data, None, None, 0, C.byref(t)) == ERR_UNSUPPORTED
    assert mw._L.edynhip_query_aabb_submit(ctx, 1, box.ctypes.data, want.ctypes.data, 64, 0, C.byref(t)) == ERR_UNSUPPORTED
    mw.close()
