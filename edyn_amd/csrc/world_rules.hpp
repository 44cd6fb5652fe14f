// The host rules of the multi-device world (multi.hpp, multi*.hip), each written once: which island a body belongs to before a device has said
// so, which shard an island, a body, a joint or an exclusion pair lives on, and when a partition is given up for a balanced one.
// Pure functions over arrays and small structs - no HIP, no context, no world - so every rule is tested on a machine without a GPU
// (tests/cpp/world_rules.cpp; the partitioner and the box sweep also through the C-ABI, tests/test_partition.py).
#pragma once
#include "../../include/edynhip.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace eh {

constexpr float kCreationMargin = 0.026f;   // broadphase.hpp:18: a manifold exists once two AABBs are this close; both boxes are grown by it
constexpr float kHorizon = 1.0f;            // cross-shard pairs further apart than this are not tracked individually

// ------------------------------------------------------------------------------------------------ island index
// The islands of the dynamic bodies: their labels sorted and unique, where a label sits among them, and the islands' summed weights.
struct IslandIndex {
    std::vector<uint32_t> isl;
    IslandIndex(uint32_t n, const uint32_t *labels, const int32_t *kind) {
        for (uint32_t i = 0; i < n; ++i) if (kind[i] == EDYNHIP_KIND_DYNAMIC) isl.push_back(labels[i]);
        std::sort(isl.begin(), isl.end());
        isl.erase(std::unique(isl.begin(), isl.end()), isl.end());
    }
    uint32_t size() const { return (uint32_t)isl.size(); }
    uint32_t index_of(uint32_t label) const { return (uint32_t)(std::lower_bound(isl.begin(), isl.end(), label) - isl.begin()); }
    std::vector<double> weights(uint32_t n, const uint32_t *labels, const int32_t *kind, const double *w_body) const {   // (summed in body order)
        std::vector<double> w(isl.size(), 0.0);
        for (uint32_t i = 0; i < n; ++i) if (kind[i] == EDYNHIP_KIND_DYNAMIC) w[index_of(labels[i])] += w_body ? w_body[i] : 1.0;
        return w;
    }
};

// Union-find whose root is the set's lowest index - the label the device's island stage gives a component.
struct LowestRoot {
    std::vector<uint32_t> parent;
    explicit LowestRoot(uint32_t n) : parent(n) { std::iota(parent.begin(), parent.end(), 0u); }
    uint32_t find(uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; }
    void unite(uint32_t a, uint32_t b) { const uint32_t ra = find(a), rb = find(b); if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb); }
};

// ------------------------------------------------------------------------------------------------ partitioners
// Longest-processing-time-first: islands by descending weight (ties: ascending label), each to the lightest rank so far (ties: the
// lowest rank). rank_of[i] = -1 for bodies that are not dynamic (replicated on every rank).
static inline void partition_islands(uint32_t n, const uint32_t *labels, const int32_t *kind, const double *weights, uint32_t world_size, int32_t *rank_of) {
    for (uint32_t i = 0; i < n; ++i) rank_of[i] = -1;
    const IslandIndex ix(n, labels, kind);
    const uint32_t m = ix.size();
    if (m == 0) return;
    const std::vector<double> w = ix.weights(n, labels, kind, weights);
    std::vector<uint32_t> order(m);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return w[a] != w[b] ? w[a] > w[b] : ix.isl[a] < ix.isl[b]; });
    std::vector<double> load(world_size, 0.0);
    std::vector<int32_t> owner(m, 0);
    for (uint32_t k : order) {
        uint32_t r = 0;
        for (uint32_t q = 1; q < world_size; ++q) if (load[q] < load[r]) r = q;
        owner[k] = (int32_t)r;
        load[r] += w[k];
    }
    for (uint32_t i = 0; i < n; ++i) if (kind[i] == EDYNHIP_KIND_DYNAMIC) rank_of[i] = owner[ix.index_of(labels[i])];
}

// The world's own placement rule (round 5): islands in the order of a space-filling curve through their box centres (30-bit Morton
// keys over the scene's bounds), cut into world_size runs of equal weight. Neighbours in space mostly share a shard, so islands that
// meet later mostly meet inside a shard - the longest-processing-time rule above scatters neighbours over the shards, and every meeting
// of two of them then costs a re-partition (a field of collapsing piles: 18 in 40 steps). A shard's load is within one island of the mean.
// aabb6[n][6]: the bodies' boxes; shapeless bodies count with a point at the origin of their island's other bodies (or 0).
static inline void partition_islands_spatial(uint32_t n, const uint32_t *labels, const int32_t *kind, const double *weights, const float *aabb6, uint32_t world_size, int32_t *rank_of) {
    for (uint32_t i = 0; i < n; ++i) rank_of[i] = -1;
    const IslandIndex ix(n, labels, kind);
    const uint32_t m = ix.size();
    if (m == 0) return;
    std::vector<double> w(m, 0.0), cx(3 * (size_t)m, 0.0), cw(m, 0.0);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t i = 0; i < n; ++i) {
        if (kind[i] != EDYNHIP_KIND_DYNAMIC) continue;
        const uint32_t k = ix.index_of(labels[i]);
        w[k] += weights ? weights[i] : 1.0;   // (IslandIndex::weights, in the pass that looks the island up anyway)
        const float *b = aabb6 + 6 * (size_t)i;
        bool finite = true;
        for (int d = 0; d < 6; ++d) finite = finite && std::isfinite(b[d]) && std::fabs(b[d]) < 1.0e30f;
        if (!finite || (b[0] == 0 && b[3] == 0 && b[1] == 0 && b[4] == 0 && b[2] == 0 && b[5] == 0)) continue;   // no shape: no place of its own
        for (int d = 0; d < 3; ++d) { cx[3 * (size_t)k + d] += 0.5 * ((double)b[d] + (double)b[3 + d]); }
        cw[k] += 1.0;
    }
    // islands without any shaped body have no place: they stay out of the bounds the Morton keys are quantised over (a scene far from the
    // origin would otherwise lose its resolution to a phantom island at 0,0,0) and take the key of the scene's lower corner
    for (uint32_t k = 0; k < m; ++k) for (int d = 0; d < 3; ++d) {
        if (cw[k] <= 0) continue;
        cx[3 * (size_t)k + d] /= cw[k];
        lo[d] = std::min(lo[d], cx[3 * (size_t)k + d]); hi[d] = std::max(hi[d], cx[3 * (size_t)k + d]);
    }
    for (uint32_t k = 0; k < m; ++k) if (cw[k] <= 0) for (int d = 0; d < 3; ++d) cx[3 * (size_t)k + d] = lo[d] <= hi[d] ? lo[d] : 0.0;
    for (int d = 0; d < 3; ++d) if (lo[d] > hi[d]) lo[d] = hi[d] = 0.0;
    auto spread = [](uint32_t v) { v &= 0x3FFu; v = (v | (v << 16)) & 0x030000FFu; v = (v | (v << 8)) & 0x0300F00Fu; v = (v | (v << 4)) & 0x030C30C3u; v = (v | (v << 2)) & 0x09249249u; return v; };
    std::vector<uint32_t> key(m), order(m);
    for (uint32_t k = 0; k < m; ++k) {
        uint32_t q[3];
        for (int d = 0; d < 3; ++d) { const double ext = hi[d] - lo[d]; q[d] = ext > 0 ? (uint32_t)std::min(1023.0, (cx[3 * (size_t)k + d] - lo[d]) / ext * 1024.0) : 0u; }
        key[k] = spread(q[0]) | (spread(q[1]) << 1) | (spread(q[2]) << 2);
    }
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : ix.isl[a] < ix.isl[b]; });
    double total = 0, before = 0;
    for (double x : w) total += x;
    std::vector<int32_t> owner(m, 0);
    for (uint32_t k : order) {   // the run an island falls into is decided by the middle of its own weight interval
        const double mid = before + 0.5 * w[k];
        owner[k] = (int32_t)std::min<double>(world_size - 1, std::floor(mid / total * world_size));
        before += w[k];
    }
    for (uint32_t i = 0; i < n; ++i) if (kind[i] == EDYNHIP_KIND_DYNAMIC) rank_of[i] = owner[ix.index_of(labels[i])];
}

// ------------------------------------------------------------------------------------------------ box sweep
struct IslandBox { float lo[3], hi[3]; uint32_t label; int32_t owner; };
// Sweep along x over boxes grown by `reach` on every side: calls hit(a, b, gap) for every pair whose grown boxes overlap, gap = the
// largest per-axis distance between the ORIGINAL boxes (0 when they overlap). cross_only: pairs of different owners only.
template <typename Hit>
static void sweep_boxes(std::vector<IslandBox> &boxes, float reach, bool cross_only, Hit &&hit) {
    // Sweep along x; the boxes still open at the sweep front are kept in BUCKETS along z, so a box only meets the open boxes of the z
    // cells it reaches. (Round 6: with one list of open boxes a field of piles on a 64 x 64 grid - 262 144 body boxes, every pile of a
    // column open at once - cost ~260 M pair tests, 0.8 s of every re-partition's 1.2 s.) A pair that shares several cells is tested in
    // the first of them only.
    std::sort(boxes.begin(), boxes.end(), [](const IslandBox &a, const IslandBox &b) { return a.lo[0] != b.lo[0] ? a.lo[0] < b.lo[0] : a.label < b.label; });
    const uint32_t nb = (uint32_t)boxes.size();
    if (nb < 2) return;
    float zlo = 3.0e38f, zhi = -3.0e38f;
    double ext = 0;
    uint32_t finite = 0;
    for (const IslandBox &b : boxes) {
        if (!(b.lo[2] <= b.hi[2]) || !std::isfinite(b.lo[2]) || !std::isfinite(b.hi[2])) continue;
        zlo = std::min(zlo, b.lo[2]); zhi = std::max(zhi, b.hi[2]); ext += (double)b.hi[2] - (double)b.lo[2]; ++finite;
    }
    const float mean_ext = finite ? (float)(ext / finite) : 0.0f;
    const float span = finite ? zhi - zlo : 0.0f;
    const uint32_t cells = span > 0 ? (uint32_t)std::min(4096.0f, std::max(1.0f, span / std::max(mean_ext + 2 * reach, 1e-3f))) : 1u;
    const float inv = cells > 1 ? (float)cells / span : 0.0f;
    auto cell_of = [&](float z) { if (!(z > zlo)) return 0u; const float c = (z - zlo) * inv; return c >= (float)(cells - 1) ? cells - 1 : (uint32_t)c; };   // (NaN and -inf land in cell 0, +inf in the last)
    std::vector<std::vector<uint32_t>> open(cells);
    std::vector<uint32_t> first_cell(nb);
    for (uint32_t k = 0; k < nb; ++k) {
        const IslandBox &bk = boxes[k];
        const bool sane = bk.lo[2] <= bk.hi[2];
        const uint32_t q0 = sane ? cell_of(bk.lo[2] - 2 * reach) : 0u, q1 = sane ? cell_of(bk.hi[2] + 2 * reach) : cells - 1;
        for (uint32_t c = q0; c <= q1; ++c) {
            std::vector<uint32_t> &bucket = open[c];
            size_t keep = 0;
            for (uint32_t a : bucket) {
                const IslandBox &ba = boxes[a];
                if (!(ba.hi[0] + 2 * reach >= bk.lo[0])) continue;   // the sweep front has passed it: drop it from this bucket
                bucket[keep++] = a;
                if (c != std::max(first_cell[a], q0)) continue;       // this pair is tested in the first cell the two share
                if (cross_only && ba.owner == bk.owner) continue;
                float gap = 0;
                for (int d = 0; d < 3; ++d) gap = std::max(gap, std::max(bk.lo[d] - ba.hi[d], ba.lo[d] - bk.hi[d]));
                if (gap < 2 * reach) hit(ba, bk, gap);
            }
            bucket.resize(keep);
        }
        const uint32_t i0 = sane ? cell_of(bk.lo[2]) : 0u, i1 = sane ? cell_of(bk.hi[2]) : cells - 1;
        first_cell[k] = i0;
        for (uint32_t c = i0; c <= i1; ++c) open[c].push_back(k);
    }
}

// The approach check's verdict over the island boxes of all shards: the smallest gap between boxes of different owners within the
// horizon. close: islands of different shards are within the creation margin of each other (also for a NaN gap); otherwise `budget`
// is how far they may still approach.
static inline void approach_verdict(std::vector<IslandBox> &boxes, bool &close, float &budget) {
    float gmin = kHorizon;
    sweep_boxes(boxes, 0.5f * kHorizon, true, [&](const IslandBox &, const IslandBox &, float gap) { gmin = std::min(gmin, gap); });
    close = !(gmin >= 2 * kCreationMargin);   // also true for NaN
    budget = close ? 0.0f : gmin - 2 * kCreationMargin;
}

// (owner << 32) | other of a manifold's body pair: the owner is the dynamic body, the higher index of two
static inline uint64_t canonical_key(const int32_t *kind, uint32_t a, uint32_t b) {
    const bool da = kind[a] == EDYNHIP_KIND_DYNAMIC, db = kind[b] == EDYNHIP_KIND_DYNAMIC;
    const uint32_t owner = (da && db) ? std::max(a, b) : (da ? a : b), other = owner == a ? b : a;
    return ((uint64_t)owner << 32) | other;
}

// ------------------------------------------------------------------------------------------------ host island estimate
// Radius of a sphere about a mesh's vertex mean that covers the hull from any point inside it (the centroid the library shifts to lies
// inside the hull: twice the radius about the mean covers it). v[nv][3].
static inline float mesh_bounding_radius(const float *v, size_t nv) {
    double c[3] = {0, 0, 0}, r2 = 0;
    for (size_t i = 0; i < nv; ++i) for (int d = 0; d < 3; ++d) c[d] += v[3 * i + d];
    for (int d = 0; d < 3; ++d) c[d] /= (double)std::max<size_t>(nv, 1);
    for (size_t i = 0; i < nv; ++i) { double q = 0; for (int d = 0; d < 3; ++d) q += (v[3 * i + d] - c[d]) * (v[3 * i + d] - c[d]); r2 = std::max(r2, q); }
    return 2.0f * (float)std::sqrt(r2);
}

// The meshes of a scene as the rules see them (vertices only); a mesh's radius is computed when it is first asked for.
struct MeshRadii {
    struct Mesh { const float *v; size_t nv; };
    std::vector<Mesh> meshes;
    std::vector<float> radius;   // negative: not computed yet
    void add(const float *v, size_t nv) { meshes.push_back({v, nv}); radius.push_back(-1.0f); }
    size_t size() const { return meshes.size(); }
    float of(size_t id) { if (radius[id] < 0) radius[id] = mesh_bounding_radius(meshes[id].v, meshes[id].nv); return radius[id]; }
};

// Radius of a sphere about the body's position that holds its shape; negative: no shape (or a plane, which is never dynamic in a
// sensible scene), touches nothing; 0 for a mesh id the scene does not hold. p: the four shape parameters; com (or nullptr): the offset
// of the centre of mass, whose length is added.
static inline float bounding_radius(MeshRadii &meshes, int shape_type, const float *p, const float *com) {
    float r = -1.0f;
    switch (shape_type) {
    case EDYNHIP_SHAPE_BOX: r = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]); break;
    case EDYNHIP_SHAPE_SPHERE: r = p[0]; break;
    case EDYNHIP_SHAPE_CAPSULE: r = p[0] + p[1]; break;
    case EDYNHIP_SHAPE_CYLINDER: r = std::sqrt(p[0] * p[0] + p[1] * p[1]); break;
    case EDYNHIP_SHAPE_POLYHEDRON: { const size_t id = (size_t)p[0]; r = id < meshes.size() ? meshes.of(id) : 0.0f; break; }
    default: return -1.0f;
    }
    if (r < 0) return r;
    if (com) r += std::sqrt(com[0] * com[0] + com[1] * com[1] + com[2] * com[2]);
    return r;
}

// n bodies as the island estimate reads them (com, jalive: optional)
struct EstimateBodies {
    uint32_t n;
    const int32_t *kind, *shape_type;
    const float *shape_param, *pos, *com;
};

// The islands of a described state, estimated on the host. An island edge exists once a manifold exists (constraint_util.cpp:76-78:
// every manifold owns a null_constraint edge), i.e. once two AABBs come within the creation margin (broadphase.hpp:15-18), or through a
// joint (island_manager.cpp:117-247). A partition only has to keep every TRUE island on one shard, so a conservative edge set is as good
// as the exact one - it merely co-locates islands that are about to meet anyway: every dynamic shaped body gets the box of its bounding
// sphere (no collision filters, no exclusions applied), boxes within the margin and jointed dynamic bodies (nj joints, jbody[nj][2],
// jalive[nj] or nullptr = all) are united, the label of a component is its lowest body index, as on the device.
// labels[n]; aabb6 (or nullptr): [n][6], the boxes used, zeros for bodies without one.
static inline void estimate_islands(const EstimateBodies &b, MeshRadii &meshes, uint32_t nj, const uint32_t *jbody, const uint8_t *jalive, uint32_t *labels, float *aabb6) {
    std::vector<IslandBox> boxes;
    if (aabb6) std::fill(aabb6, aabb6 + 6 * (size_t)b.n, 0.0f);
    for (uint32_t i = 0; i < b.n; ++i) {
        if (b.kind[i] != EDYNHIP_KIND_DYNAMIC) continue;
        const float r = bounding_radius(meshes, b.shape_type[i], b.shape_param + 4 * (size_t)i, b.com ? b.com + 3 * (size_t)i : nullptr);
        if (r < 0) continue;
        IslandBox box;
        for (int d = 0; d < 3; ++d) { box.lo[d] = b.pos[3 * (size_t)i + d] - r; box.hi[d] = b.pos[3 * (size_t)i + d] + r; }
        if (aabb6) for (int d = 0; d < 3; ++d) { aabb6[6 * (size_t)i + d] = box.lo[d]; aabb6[6 * (size_t)i + 3 + d] = box.hi[d]; }
        box.label = i; box.owner = 0;
        boxes.push_back(box);
    }
    LowestRoot uf(b.n);
    sweep_boxes(boxes, kCreationMargin, false, [&](const IslandBox &x, const IslandBox &y, float) { uf.unite(x.label, y.label); });
    for (uint32_t g = 0; g < nj; ++g) {
        if (jalive && !jalive[g]) continue;
        const uint32_t a = jbody[2 * g], c = jbody[2 * g + 1];
        if (b.kind[a] == EDYNHIP_KIND_DYNAMIC && b.kind[c] == EDYNHIP_KIND_DYNAMIC) uf.unite(a, c);
    }
    for (uint32_t i = 0; i < b.n; ++i) labels[i] = uf.find(i);
}

// ------------------------------------------------------------------------------------------------ welding
// The box of every island: the union of the AABBs (aabb6[n][6]) of its shaped dynamic bodies (a shapeless body touches nothing), in
// ascending label order, owner 0. An island without a shaped body keeps an inverted box.
static inline std::vector<IslandBox> island_boxes_of(uint32_t n, const uint32_t *labels, const int32_t *kind, const int32_t *shape_type, const float *aabb6) {
    const IslandIndex ix(n, labels, kind);
    std::vector<IslandBox> boxes(ix.size());
    for (size_t k = 0; k < boxes.size(); ++k) { for (int d = 0; d < 3; ++d) { boxes[k].lo[d] = 3.0e38f; boxes[k].hi[d] = -3.0e38f; } boxes[k].label = ix.isl[k]; boxes[k].owner = 0; }
    for (uint32_t i = 0; i < n; ++i) {
        if (kind[i] != EDYNHIP_KIND_DYNAMIC || shape_type[i] == EDYNHIP_SHAPE_NONE) continue;
        IslandBox &b = boxes[ix.index_of(labels[i])];
        for (int d = 0; d < 3; ++d) { b.lo[d] = std::min(b.lo[d], aabb6[6 * (size_t)i + d]); b.hi[d] = std::max(b.hi[d], aabb6[6 * (size_t)i + 3 + d]); }
    }
    return boxes;
}

// The islands that have to share a shard, welded: islands whose boxes overlap (grown by the creation margin) - all such pairs, also
// those the last partition had co-located (they may still be separate islands, and the partitioner would be free to split them) - and
// islands tied by an edge between two dynamic bodies. The labels may be stale (a shard that has not stepped since it was built still
// has the labels it was built with), but the edges the island manager connects bodies through are known on the host - every live
// joint, every pair an edit is about to join, every carried manifold (island_manager.cpp:117-247) - so they are united whatever the
// labels say: a joint or a carried manifold can never end up with its bodies on two shards.
// pairs: the edges, each a span of `count` records whose two body indices sit `stride` bytes apart from record to record.
struct EdgeSpan { const void *first; size_t stride, count; const uint8_t *alive; };   // first -> uint32_t[2]; alive (or nullptr): per record
// boxes (out): the islands' boxes BEFORE welding, sorted by the sweep. Returns welded[n]: per body the lowest label of its group.
static inline std::vector<uint32_t> weld_islands(uint32_t n, const uint32_t *labels, const int32_t *kind, const int32_t *shape_type, const float *aabb6,
                                          const std::vector<EdgeSpan> &edges, std::vector<IslandBox> &boxes) {
    boxes = island_boxes_of(n, labels, kind, shape_type, aabb6);
    LowestRoot uf(n);
    for (const EdgeSpan &e : edges)
        for (size_t k = 0; k < e.count; ++k) {
            if (e.alive && !e.alive[k]) continue;
            const uint32_t *ab = (const uint32_t *)((const uint8_t *)e.first + k * e.stride);
            if (kind[ab[0]] != EDYNHIP_KIND_DYNAMIC || kind[ab[1]] != EDYNHIP_KIND_DYNAMIC) continue;
            uf.unite(labels[ab[0]], labels[ab[1]]);
        }
    sweep_boxes(boxes, kCreationMargin, false, [&](const IslandBox &a, const IslandBox &b, float) { uf.unite(a.label, b.label); });
    std::vector<uint32_t> welded(n);
    for (uint32_t i = 0; i < n; ++i) welded[i] = uf.find(labels[i]);
    return welded;
}

// ------------------------------------------------------------------------------------------------ sticky moves and the rebalance
// Sticky: a group (welded[n]) that spans shards goes to the shard holding most of its dynamic bodies (ties: the lower shard);
// everybody else stays where rank_of[n] has them.
static inline std::vector<int32_t> sticky_targets(uint32_t n, const uint32_t *welded, const int32_t *kind, const int32_t *rank_of, uint32_t W) {
    std::vector<int32_t> next(rank_of, rank_of + n);
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; ++i) if (kind[i] == EDYNHIP_KIND_DYNAMIC) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return welded[a] != welded[b] ? welded[a] < welded[b] : a < b; });
    std::vector<uint32_t> count(W);
    for (size_t a = 0; a < order.size();) {
        size_t e = a;
        std::fill(count.begin(), count.end(), 0u);
        while (e < order.size() && welded[order[e]] == welded[order[a]]) { ++count[(uint32_t)rank_of[order[e]]]; ++e; }
        uint32_t target = 0, spans = 0;
        for (uint32_t r = 0; r < W; ++r) { if (count[r]) ++spans; if (count[r] > count[target]) target = r; }
        if (spans > 1) for (size_t k = a; k < e; ++k) next[order[k]] = (int32_t)target;
        a = e;
    }
    return next;
}

// Sticky moves only ever add to the shard that holds most of a group: a collapsing or merging scene would drift onto a few shards.
// Once the heaviest shard carries more than 1.5 x the mean (of a world of at least 8 bodies per shard), the meeting takes the full,
// spatially balanced re-partition instead (the price is one rebuild of every shard, the gain every later step of the
// slowest shard).
static inline bool needs_rebalance(uint32_t n, const int32_t *rank_of, uint32_t W) {
    if (W <= 1) return false;
    std::vector<uint32_t> load(W, 0);
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; ++i) if (rank_of[i] >= 0) { ++load[(uint32_t)rank_of[i]]; ++total; }
    const uint32_t heaviest = *std::max_element(load.begin(), load.end());
    return total >= 8 * W && (double)heaviest * W > 1.5 * (double)total;
}

// ------------------------------------------------------------------------------------------------ new bodies
// Placement of n new bodies, one after the other in index order: replicated (-1), or the shard with the fewest live dynamic bodies
// (load[W], updated; ties: the lowest shard) - and with a body every later body of the call that it touches, directly or through
// others (group[n]: the lowest index of its group, placed before its members): a pile spawned in one call lands on one shard instead
// of being welded together there. extra[W] (added to): the bodies every shard's context has to take, replicas included.
static inline std::vector<int32_t> place_new_bodies(uint32_t n, const int32_t *kind, const uint32_t *group, std::vector<uint32_t> &load, std::vector<uint32_t> &extra) {
    const uint32_t W = (uint32_t)load.size();
    std::vector<int32_t> place(n, -1);
    for (uint32_t k = 0; k < n; ++k) {
        if (kind[k] != EDYNHIP_KIND_DYNAMIC) { for (uint32_t r = 0; r < W; ++r) ++extra[r]; continue; }
        uint32_t r = 0;
        if (group[k] != k) r = (uint32_t)place[group[k]];
        else for (uint32_t q = 1; q < W; ++q) if (load[q] < load[r]) r = q;
        place[k] = (int32_t)r; ++load[r]; ++extra[r];
    }
    return place;
}

// ------------------------------------------------------------------------------------------------ ownership
// rank: a body's shard, negative = replicated on every shard.
// Shard r holds a body's state in its context when it owns it or the body is replicated ...
static inline bool shard_holds_body(int32_t rank, uint32_t r) { return rank == (int32_t)r || rank < 0; }
// ... and reports it (state, queries, records) when it owns it; shard 0 also reports the replicated ones.
static inline bool shard_reports_body(int32_t rank, uint32_t r) { return rank == (int32_t)r || (rank < 0 && r == 0); }
// The rank a body of this kind counts with where it matters who owns it: only a dynamic body has an owner.
static inline int32_t owner_rank(int32_t kind, int32_t rank) { return kind == EDYNHIP_KIND_DYNAMIC ? rank : -1; }
// The shard a joint between bodies on ranks ra, rb lives on: the one that owns a body of it (a joint to a replicated anchor lives on
// one shard). -1: both replicated - no context holds it; -2: two shards - a joint is an island edge, a partition must never do that.
static inline int32_t joint_home(int32_t ra, int32_t rb) {
    if (ra >= 0 && rb >= 0) return ra == rb ? ra : -2;
    return ra >= 0 ? ra : (rb >= 0 ? rb : -1);
}
// Shard r holds the exclusion of a pair when it holds both bodies and owns one of them: one shard when an owner is involved and both
// are there, none for a pair of two shards (the scene's until its bodies meet) or of two replicated bodies.
static inline bool shard_holds_exclusion(int32_t ra, int32_t rb, uint32_t r) {
    return shard_holds_body(ra, r) && shard_holds_body(rb, r) && (ra == (int32_t)r || rb == (int32_t)r);
}

// ------------------------------------------------------------------------------------------------ materials
// contact_extras materials, material ids and the mix table on a multi-device world (multi_materials.hip). What a contact point carries
// beyond edynhip_manifold - its material as mixed at creation and the warm-start impulses of its rolling pair and spinning row - travels
// through a re-partition as one 128-byte row per manifold: row[2 k .. 2 k + 1] of point k = (roll, spin, stiffness, damping),
// (rolling impulse 0, 1, spin impulse, -), four floats each; the slots at or beyond the manifold's point count are all zero.
constexpr float kMaterialLarge = 1e18f;        // large_scalar: the default stiffness and damping (dmath.hpp kLarge)
constexpr uint32_t kUnassignedMaterial = 0xFFFFu;
constexpr uint32_t kExtrasRowFloats = 32;
// material::{spin_friction, roll_friction, stiffness, damping} as a body is created with them (comp/material.hpp:15-22)
static inline bool material_extras_default(float spin, float roll, float stiffness, float damping) {
    return !(spin > 0) && !(roll > 0) && !(stiffness < kMaterialLarge) && !(damping < kMaterialLarge);
}
static inline bool material_extras_valid(float spin, float roll, float stiffness, float damping) {
    return !(spin < 0) && !(roll < 0) && stiffness > 0 && damping > 0;
}
// The row of a manifold whose context keeps no extras: every living point has the default material and no impulses.
static inline void extras_row_default(float *row, uint32_t num_points) {
    for (uint32_t i = 0; i < kExtrasRowFloats; ++i) row[i] = 0.0f;
    for (uint32_t k = 0; k < num_points && k < 4; ++k) { row[8 * k + 2] = kMaterialLarge; row[8 * k + 3] = kMaterialLarge; }
}
// ... and whether a row says no more than that: a shard that is given only such rows needs no extras storage of its own.
static inline bool extras_row_is_default(const float *row, uint32_t num_points) {
    for (uint32_t k = 0; k < num_points && k < 4; ++k) {
        const float *p = row + 8 * k;
        if (p[0] != 0 || p[1] != 0 || p[2] != kMaterialLarge || p[3] != kMaterialLarge || p[4] != 0 || p[5] != 0 || p[6] != 0) return false;
    }
    return true;
}
// edynhip_get_point_extras' 4 x 7 floats of a manifold from its row: rolling impulse[2], spin impulse, roll, spin, stiffness, damping
static inline void extras_row_to_out7(const float *row, float *out28) {
    for (uint32_t k = 0; k < 4; ++k) {
        const float *p = row + 8 * k;
        float *o = out28 + 7 * k;
        o[0] = p[4]; o[1] = p[5]; o[2] = p[6]; o[3] = p[0]; o[4] = p[1]; o[5] = p[2]; o[6] = p[3];
    }
}
// The shards that take an edit of the bodies [first, first + n): the owner of a dynamic body, every shard for a replicated one.
// touched[W] (cleared first); rank_of as the partition has it.
static inline void shards_of_body_range(const int32_t *rank_of, uint32_t first, uint32_t n, uint32_t W, uint8_t *touched) {
    for (uint32_t r = 0; r < W; ++r) touched[r] = 0;
    for (uint32_t i = first; i < first + n; ++i) {
        if (rank_of[i] >= 0) { if ((uint32_t)rank_of[i] < W) touched[(uint32_t)rank_of[i]] = 1; }
        else for (uint32_t r = 0; r < W; ++r) touched[r] = 1;
    }
}
// A re-partition carries the points' extras once the world holds any contact_extras material or any mix-table entry: from then on a
// point may have been created with a mix that today's materials would not give it again. A world without either carries nothing.
static inline bool extras_carry_needed(bool any_extras_material_ever, size_t mix_entries) { return any_extras_material_ever || mix_entries != 0; }

// ------------------------------------------------------------------------------------------------ body edits
// edynhip_world_edit_bodies (multi_body_edit.hip). Shard r takes the edit of a body that is dynamic BEFORE the edit when it owns it, of a
// replicated one always: an edit goes to every context that holds the body.
static inline bool shard_takes_body_edit(int32_t kind_before, int32_t rank, uint32_t r) { return shard_holds_body(owner_rank(kind_before, rank), r); }
// An edit crosses the replication boundary when its kind changes between dynamic and not dynamic: the body changes who holds it.
static inline bool edit_crosses_boundary(int32_t kind_before, int32_t kind_after) {
    return (kind_before == EDYNHIP_KIND_DYNAMIC) != (kind_after == EDYNHIP_KIND_DYNAMIC);
}
// The kind a body has after an edit of the groups `fields` that names `kind_given` for it
static inline int32_t kind_after_edit(uint32_t fields, int32_t kind_before, int32_t kind_given) { return (fields & EDYNHIP_EDIT_KIND) ? kind_given : kind_before; }
// The shard a body made dynamic goes to: the one with the fewest live dynamic bodies (load[W], updated), ties to the lowest shard -
// place_new_bodies' rule for a body that touches no other of its call.
static inline uint32_t owner_of_new_dynamic(std::vector<uint32_t> &load) {
    uint32_t r = 0;
    for (uint32_t q = 1; q < (uint32_t)load.size(); ++q) if (load[q] < load[r]) r = q;
    ++load[r];
    return r;
}
// A context keeps the inertia it derived from the shape a body HAD when only the shape is edited; a shard rebuilt from the scene would
// derive it from the new one. So before a SHAPE edit without INERTIA lands in the scene, the inertia the scene still leaves to the old
// shape is written out (dbodyinit.hpp shape_inertia, the same float operations in the same order: the inverse the context takes of it is
// the same bits). Boxes and spheres without a centre-of-mass offset; false: another shape - the scene keeps deriving (DESIGN, not covered).
static inline bool bake_shape_inertia(int32_t shape_type, const float *p, float mass, bool has_com, float *inertia9) {
    if (has_com) return false;
    float d[3];
    if (shape_type == EDYNHIP_SHAPE_BOX) {
        const float ex = p[0] * 2.0f, ey = p[1] * 2.0f, ez = p[2] * 2.0f, c = 1.0f / 12.0f * mass;
        d[0] = c * (ey * ey + ez * ez); d[1] = c * (ez * ez + ex * ex); d[2] = c * (ex * ex + ey * ey);
    } else if (shape_type == EDYNHIP_SHAPE_SPHERE) {
        const float s = 0.4f * mass * p[0] * p[0];
        d[0] = d[1] = d[2] = s;
    } else return false;
    for (int k = 0; k < 9; ++k) inertia9[k] = 0.0f;
    inertia9[0] = d[0]; inertia9[4] = d[1]; inertia9[8] = d[2];
    return true;
}
// An edit makes the approach check due at once when it can bring islands of two shards within the creation margin before the next step: a
// new shape on a body that is dynamic afterwards, or a body made dynamic. A replicated body is on every shard already; a world of one
// shard has nobody to approach.
static inline bool edit_needs_approach_check(uint32_t fields, int32_t kind_before, int32_t kind_after, uint32_t W) {
    if (W < 2 || kind_after != EDYNHIP_KIND_DYNAMIC) return false;
    return (fields & EDYNHIP_EDIT_SHAPE) != 0 || kind_before != EDYNHIP_KIND_DYNAMIC;
}

}  // namespace eh
