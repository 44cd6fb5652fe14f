"""The definition of the AABB queries (edynhip_query_aabb) in numpy, for the tests to compare the device against.

A candidate box is reported for a query q iff intersect_aabb(q.min, q.max, box.min - 0.1, box.max + 0.1): the reference's six
comparisons on closed intervals (include/edyn/comp/aabb.hpp:45-47, src/edyn/math/geom.cpp:762-770) against the box a freshly created
leaf of the reference's dynamic_tree holds (aabb.inset(aabb_inset), aabb_inset = -0.1: include/edyn/collision/dynamic_tree.hpp:24,
src/edyn/collision/dynamic_tree.cpp:45; the walk: dynamic_tree.cpp query, include/edyn/collision/query_tree.hpp:36-42). The inset is a
float32 operation (box.min + -0.1f, box.max - -0.1f), the comparisons are evaluated as written: touching is a hit, a NaN fails every
comparison, an inverted query is not special. Hits come in ascending id per query (the one difference from the reference, which
reports in tree-visit order)."""
import numpy as np

INSET = np.float32(0.1)


def fat(boxes):
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    return (b[:, :3] - INSET).astype(np.float32), (b[:, 3:] + INSET).astype(np.float32)


def query(boxes, queries, ids=None, chunk=1 << 24):
    """boxes [m][6], queries [n][6] (min, max), ids [m] (default 0 .. m-1, must ascend) -> (offsets uint32 [n + 1], ids uint32 [total])."""
    fmin, fmax = fat(boxes)
    q = np.asarray(queries, np.float32).reshape(-1, 6)
    ids = np.arange(len(fmin), dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)
    assert len(ids) == len(fmin) and (len(ids) < 2 or np.all(ids[1:] > ids[:-1]))
    counts = np.zeros(len(q), np.int64)
    out = []
    step = max(1, chunk // max(1, len(fmin)))
    with np.errstate(invalid="ignore"):
        for s in range(0, len(q), step):
            qq = q[s:s + step]
            hit = np.ones((len(qq), len(fmin)), bool)
            for d in range(3):
                hit &= (qq[:, d, None] <= fmax[None, :, d]) & (qq[:, 3 + d, None] >= fmin[None, :, d])
            counts[s:s + step] = hit.sum(axis=1)
            out.append(ids[np.nonzero(hit)[1]])   # row-major: by query, ascending candidate
    offsets = np.zeros(len(q) + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    return offsets, (np.concatenate(out) if out else np.zeros(0, np.uint32)).astype(np.uint32)


def split_tree_hits(hits, n):
    """oracle.binding.tree_run's hit stream (each query terminated by 0xFFFFFFFF) -> (offsets, ids sorted ascending per query)."""
    hits = np.asarray(hits, np.uint32)
    ends = np.flatnonzero(hits == 0xFFFFFFFF)
    assert len(ends) == n and (len(hits) == 0 or ends[-1] == len(hits) - 1)
    starts = np.concatenate([[0], ends[:-1] + 1])
    counts = ends - starts
    qidx = np.repeat(np.arange(n), counts)
    vals = hits[hits != 0xFFFFFFFF]
    order = np.lexsort((vals, qidx))
    offsets = np.zeros(n + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    return offsets, vals[order].astype(np.uint32)
