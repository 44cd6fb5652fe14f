"""The definition the device's AABB queries are held to (tests/query_ref.py) against the reference's own dynamic_tree: on a tree whose
leaves were just created, dynamic_tree::query reports exactly the boxes that pass intersect_aabb against the box grown by 0.1 - touching
faces, degenerate, all-containing, empty and inverted queries included. No GPU needed. The real tree (oracle/_ref/libedynref.so) is
compared where it is built; the oracle's own tree (oracle/liboracle.so, checked against the real one by test_reference_engine.py) always."""
import os
import sys

import numpy as np
import pytest

from edyn_amd import scenes
from oracle import binding as ob

import query_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_query_aabb as mq   # noqa: E402
import make_raycast as mr      # noqa: E402

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(ob.__file__), "_ref", "libedynref.so"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libedynref.so is absent (built where the reference sources are)")

N_BOXES, N_QUERIES = 2000, 20000
# shares of the 20 000 queries: 1/8 each touch a fat box's max / min face exactly, each followed by its twin one ulp apart (1/4 touching +
# 1/4 twins); of the other half 5/9 are random and 1/9 each degenerate, all-containing, empty and inverted
KINDS = ("random", "touch_max", "touch_min", "degenerate", "everything", "nothing", "inverted", "twin")


def _case():
    u = scenes.splitmix64_uniform(6 * N_BOXES, stream=401).astype(np.float64).reshape(N_BOXES, 6)
    c = (u[:, :3] * 2 - 1) * 20
    h = 0.1 + u[:, 3:] * 0.9
    boxes = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    pairs = N_QUERIES // 2
    v = scenes.splitmix64_uniform(12 * pairs, stream=402).astype(np.float64).reshape(pairs, 12)
    sel = np.minimum((v[:, 0] * 16).astype(np.int64), 15)
    pick = np.minimum((v[:, 1] * N_BOXES).astype(np.int64), N_BOXES - 1)
    axis = np.minimum((v[:, 2] * 3).astype(np.int64), 2)
    t_max, twin_max = mq.touching(boxes, pick, axis, np.ones(pairs, np.int64), v[:, 3])
    t_min, twin_min = mq.touching(boxes, pick, axis, np.zeros(pairs, np.int64), v[:, 3])
    q = np.zeros((N_QUERIES, 6), np.float32)
    kind = np.zeros(N_QUERIES, np.int64)
    target = np.full(N_QUERIES, -1, np.int64)
    fmin, fmax = query_ref.fat(boxes)
    for i in range(pairs):
        a, b = 2 * i, 2 * i + 1
        if sel[i] < 8:     # a touching query and its twin
            mx = sel[i] < 4
            q[a], q[b] = (t_max[i], twin_max[i]) if mx else (t_min[i], twin_min[i])
            kind[a], kind[b] = (1 if mx else 2), 7
            target[a] = target[b] = pick[i]
            continue
        for j, e in ((a, 4), (b, 8)):
            kk = int(v[i, e] * 9)
            cc = (v[i, e + 1:e + 4] * 2 - 1) * 21
            hh = 0.05 + v[i, 5:8] * (3.0 if j == a else 0.5)
            box = np.concatenate([cc - hh, cc + hh]).astype(np.float32)
            if kk < 5:
                kind[j] = 0
            elif kk == 5:    # degenerate: zero thickness, on a fat face of the picked box
                box[:3], box[3:] = fmin[pick[i]], fmax[pick[i]]
                box[axis[i]] = box[3 + axis[i]] = fmax[pick[i], axis[i]]
                kind[j], target[j] = 3, pick[i]
            elif kk == 6:
                box = np.float32([-1e6] * 3 + [1e6] * 3); kind[j] = 4
            elif kk == 7:
                box = (box + np.float32(1000.0)).astype(np.float32); kind[j] = 5
            else:
                box[axis[i]], box[3 + axis[i]] = box[3 + axis[i]], box[axis[i]]; kind[j] = 6
            q[j] = box
    return boxes, q, kind, target


def _tree(boxes, q, real):
    ops = np.zeros((len(boxes) + len(q), 2), np.int32)
    ops[:len(boxes), 1] = np.arange(len(boxes))
    ops[len(boxes):, 0] = 3
    hits, _ = ob.tree_run(ops, np.concatenate([boxes, q]), real=real, max_hits=1 << 24)
    return query_ref.split_tree_hits(hits, len(q))


def _hits(off, ids, i, body):
    return body in ids[off[i]:off[i + 1]]


def test_the_case_holds_the_hard_queries():
    boxes, q, kind, target = _case()
    assert len(boxes) >= 2000 and len(q) >= 20000
    counts = np.bincount(kind, minlength=len(KINDS))
    assert counts[0] > 4000 and counts[1] > 1500 and counts[2] > 1500 and counts[7] == counts[1] + counts[2]
    assert all(counts[k] > 500 for k in (3, 4, 5, 6)), counts
    off, ids = query_ref.query(boxes, q)
    n_hit = np.diff(off.astype(np.int64))
    touch = np.flatnonzero((kind == 1) | (kind == 2))
    fmin, fmax = query_ref.fat(boxes)
    for i in touch:   # face equal to the fat face in float32; the twin is the next float32 away from it
        ax = int(np.flatnonzero(q[i] != q[i + 1])[0]) % 3
        if kind[i] == 1:
            assert q[i, ax] == fmax[target[i], ax] and q[i + 1, ax] == np.nextafter(q[i, ax], np.float32(np.inf))
        else:
            assert q[i, 3 + ax] == fmin[target[i], ax] and q[i + 1, 3 + ax] == np.nextafter(q[i, 3 + ax], np.float32(-np.inf))
        assert _hits(off, ids, i, target[i]) and not _hits(off, ids, i + 1, target[i]), i
    for i in np.flatnonzero(kind == 3):
        assert np.any(q[i, :3] == q[i, 3:]) and _hits(off, ids, i, target[i])
    assert np.all(n_hit[kind == 4] == len(boxes)) and np.all(n_hit[kind == 5] == 0)
    inv = kind == 6
    assert np.all(np.any(q[inv, :3] > q[inv, 3:], axis=1)) and (n_hit[inv] > 0).sum() > 0   # the formula can still report boxes


def test_definition_equals_the_oracles_tree():
    boxes, q, _, _ = _case()
    off, ids = query_ref.query(boxes, q)
    t_off, t_ids = _tree(boxes, q, real=False)
    assert np.array_equal(off, t_off) and np.array_equal(ids, t_ids)


@needs_ref
def test_definition_equals_the_real_dynamic_tree():
    boxes, q, _, _ = _case()
    off, ids = query_ref.query(boxes, q)
    t_off, t_ids = _tree(boxes, q, real=True)
    assert np.array_equal(off, t_off) and np.array_equal(ids, t_ids)


def _fixture(which):
    s = mr.scene()
    fx = np.load(os.path.join(os.path.dirname(mq.__file__), f"query_aabb_{which}.npz"))
    q = mq.queries(which, s, fx["aabb"])
    assert str(fx["scene_sha256"]) == mr.scene_digest(s) and str(fx["queries_sha256"]) == mr.digest(q)
    return s, fx, q


@pytest.mark.parametrize("which", mq.SETS)
def test_definition_reproduces_the_committed_fixtures(which):
    s, fx, q = _fixture(which)
    assert len(q) >= 4000
    for cat in mq.CATEGORIES:
        mask = mq.category_mask(s, cat)
        off, ids = query_ref.query(fx["aabb"][mask], q, ids=np.flatnonzero(mask))
        assert np.array_equal(off, fx[cat + "_offsets"]) and np.array_equal(ids, fx[cat + "_ids"]), cat
        assert off[-1] > 1000
    plane = int(np.flatnonzero(s["shape_type"] == scenes.SHAPE_PLANE)[0])
    assert (fx["non_procedural_ids"] == plane).sum() > (100 if which == "planes" else 10)
    assert plane not in fx["procedural_ids"]


@needs_ref
@pytest.mark.parametrize("which", mq.SETS)
def test_committed_fixtures_are_what_the_real_tree_returns(which):
    s, fx, q = _fixture(which)
    aabb = mq.reference_aabbs(s)
    assert np.array_equal(aabb, fx["aabb"])
    for cat in mq.CATEGORIES:
        off, ids = mq.real_tree(aabb, mq.category_mask(s, cat), q)
        assert np.array_equal(off, fx[cat + "_offsets"]) and np.array_equal(ids, fx[cat + "_ids"]), cat
