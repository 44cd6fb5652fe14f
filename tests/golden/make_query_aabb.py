"""Generates tests/golden/query_aabb_{bodies,planes}.npz: what the reference's own dynamic_tree (src/edyn/collision/dynamic_tree.cpp
create + query, compiled into oracle/_ref/libedynref.so and driven through oracle/ref_xcheck.cpp ref_tree_run) reports for two sets of
query boxes on the scene of make_raycast.scene(), built by the real engine (RefWorld) in zero gravity and stepped once. The AABBs the
engine computed are fed into freshly created leaves - one tree for the procedural (dynamic) bodies and one for the non-procedural
(static) ones, the plane included, as the reference's broadphase keeps them - so every leaf holds exactly its AABB grown by 0.1.

  bodies  queries around the lattice: of a body's size, ten times that, huge, empty, degenerate, inverted, and faces that touch a fat box
          exactly, each with a twin moved one ulp apart
  planes  queries about the plane's half-space box: above, below, across and touching its top face

The files hold recorded results only: the engine's AABBs, per category the CSR result (offsets, ids ascending per query; the reference's
visit order is not kept), and digests of the scene and the queries, which the tests rebuild bit for bit from SplitMix64 streams.

Run from the repo root (needs `make -C oracle ref`):  python tests/golden/make_query_aabb.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from edyn_amd import scenes   # noqa: E402
import make_raycast as mr     # noqa: E402
import query_ref              # noqa: E402

SETS = ("bodies", "planes")
QUERIES_PER_SET = 4000
CATEGORIES = ("procedural", "non_procedural")


def category_mask(s, category):
    shaped = s["shape_type"] != scenes.SHAPE_NONE
    dyn = s["kind"] == scenes.KIND_DYNAMIC
    return shaped & (dyn if category == "procedural" else ~dyn)


def touching(aabb, pick, axis, side, u):
    """Query boxes with one face equal to the picked fat box's face (float32), overlapping it on the other axes; and the twins one ulp
    apart. side 1: q.min = box.max + 0.1; side 0: q.max = box.min - 0.1."""
    fmin, fmax = query_ref.fat(aabb[pick])
    n = len(pick)
    c = ((fmin + fmax) * np.float32(0.5)).astype(np.float32)
    q = np.concatenate([c - np.float32(0.05), c + np.float32(0.05)], axis=1).astype(np.float32)
    r = np.arange(n)
    thick = (0.01 + u * 2.0).astype(np.float32)
    face = np.where(side == 1, fmax[r, axis], fmin[r, axis]).astype(np.float32)
    q[r, axis] = np.where(side == 1, face, face - thick)
    q[r, 3 + axis] = np.where(side == 1, face + thick, face)
    twin = q.copy()
    twin[r, axis] = np.where(side == 1, np.nextafter(face, np.float32(np.inf)), twin[r, axis])
    twin[r, 3 + axis] = np.where(side == 1, twin[r, 3 + axis], np.nextafter(face, np.float32(-np.inf)))
    return q, twin


def queries(which, s, aabb, n=QUERIES_PER_SET):
    """float32 [n][6] query boxes of one set, from the scene and the engine's AABBs."""
    k = SETS.index(which)
    u = scenes.splitmix64_uniform(12 * n, stream=300 + k).astype(np.float64).reshape(n, 12)
    bodies = np.flatnonzero((s["shape_type"] != scenes.SHAPE_PLANE) & (s["shape_type"] != scenes.SHAPE_NONE))
    pick = bodies[np.minimum((u[:, 0] * len(bodies)).astype(np.int64), len(bodies) - 1)]
    kind = np.minimum((u[:, 1] * 8).astype(np.int64), 7)
    axis = np.minimum((u[:, 2] * 3).astype(np.int64), 2)
    side = (u[:, 3] < 0.5).astype(np.int64)
    lo, hi = np.array([-10.0, -1.0, -10.0]), np.array([10.0, 9.0, 10.0])
    if which == "planes":
        plane = int(np.flatnonzero(s["shape_type"] == scenes.SHAPE_PLANE)[0])
        top = float(aabb[plane, 4])
        c = np.stack([(u[:, 4] * 2 - 1) * 12, top + (u[:, 5] * 2 - 1) * 2.0, (u[:, 6] * 2 - 1) * 12], axis=1)
        h = 0.05 + u[:, 7:10] * np.where(kind[:, None] < 4, 0.6, 6.0)
        q = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
        t, twin = touching(aabb, np.full(n, plane), np.ones(n, np.int64), np.ones(n, np.int64), u[:, 10])
        sel = kind == 6
        q[sel] = t[sel]
        sel = kind == 7
        q[sel] = twin[sel]
        return q
    c = lo + (hi - lo) * u[:, 4:7]
    h = np.where(kind[:, None] == 0, 0.25 + u[:, 7:10] * 0.5, np.where(kind[:, None] == 1, 2.5 + u[:, 7:10] * 5.0, 0.05 + u[:, 7:10] * 1.5))
    q = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    q[kind == 2] = np.float32([-1e6, -1e6, -1e6, 1e6, 1e6, 1e6])                     # everything
    sel = kind == 3
    q[sel] = (q[sel] + np.float32(500.0)).astype(np.float32)                         # nothing
    r = np.flatnonzero(kind == 4)                                                    # degenerate: zero thickness on one axis
    q[r, 3 + axis[r]] = q[r, axis[r]]
    r = np.flatnonzero(kind == 5)                                                    # inverted on one axis
    q[r, axis[r]], q[r, 3 + axis[r]] = q[r, 3 + axis[r]].copy(), q[r, axis[r]].copy()
    t, twin = touching(aabb, pick, axis, side, u[:, 10])
    q[kind == 6] = t[kind == 6]
    q[kind == 7] = twin[kind == 7]
    return q


def reference_aabbs(s):
    r = mr.reference_world(s)
    return r.get_derived()[0].astype(np.float32)


def real_tree(aabb, mask, q):
    """The real dynamic_tree: one create per box of the category (payload = body index), then the queries."""
    from oracle import binding as ob
    idx = np.flatnonzero(mask)
    ops = np.zeros((len(idx) + len(q), 2), np.int32)
    ops[:len(idx), 1] = idx
    ops[len(idx):, 0] = 3
    hits, _ = ob.tree_run(ops, np.concatenate([aabb[idx], q]), real=True, max_hits=1 << 24)
    return query_ref.split_tree_hits(hits, len(q))


def main():
    s = mr.scene()
    aabb = reference_aabbs(s)
    for which in SETS:
        q = queries(which, s, aabb)
        out = {"aabb": aabb, "queries_sha256": mr.digest(q), "scene_sha256": mr.scene_digest(s)}
        for cat in CATEGORIES:
            off, ids = real_tree(aabb, category_mask(s, cat), q)
            out[cat + "_offsets"], out[cat + "_ids"] = off, ids
        path = os.path.join(HERE, f"query_aabb_{which}.npz")
        np.savez_compressed(path, **out)
        print(which, {c: int(out[c + "_offsets"][-1]) for c in CATEGORIES}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
