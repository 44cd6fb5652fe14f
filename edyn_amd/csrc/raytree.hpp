// The query tree the raycast (raycast.hip) and the AABB queries (query_aabb.hip) share: per-body boxes from the current transforms and a
// linear BVH with ropes over every shaped non-plane body, rebuilt by query_tree_prepare at the first query after
// edynhip_ctx::state_epoch moved on. Leaves hold exactly (AABB - 0.1, AABB + 0.1), internal nodes a superset of their children.
#pragma once
#include "ctx.hpp"
#include "dmath.hpp"
#include <vector>

namespace eh {

constexpr float kFatInset = 0.1f;             // dynamic_tree::aabb_inset = -0.1 (dynamic_tree.hpp:24, dynamic_tree.cpp:45)
constexpr uint32_t kLeafBit = 0x80000000u;    // nmin.w of a leaf: kLeafBit | body; of an internal node: its left child
constexpr uint32_t kRayEnd = 0xFFFFFFFFu;     // rope of the last node of a depth-first walk (broadphase.hip kRopeEnd)

// intersect_aabb(q.min, q.max, box.min, box.max), geom.cpp:762-770: the six comparisons as written; and the box a leaf (or an island)
// is tested with, grown by the inset. One definition for every AABB query: the lists of a box ticket must agree bit for bit.
DI bool qa_overlap(dm::f3 qmn, dm::f3 qmx, dm::f3 bmn, dm::f3 bmx) {
    return (qmn.x <= bmx.x) && (qmx.x >= bmn.x) && (qmn.y <= bmx.y) && (qmx.y >= bmn.y) && (qmn.z <= bmx.z) && (qmx.z >= bmn.z);
}
DI dm::f3 qa_fat_min(float4 a) { return dm::mk3(a.x - kFatInset, a.y - kFatInset, a.z - kFatInset); }
DI dm::f3 qa_fat_max(float4 a) { return dm::mk3(a.x + kFatInset, a.y + kFatInset, a.z + kFatInset); }

struct RayTree {
    uint32_t cap = 0;
    uint64_t epoch = 0;               // edynhip_ctx::state_epoch the boxes and the tree were built for (0: never)
    uint32_t n_tree = 0, n_planes = 0;
    float4 *org = nullptr, *amin = nullptr, *amax = nullptr;   // [cap] shape frame and AABB from the current transforms
    uint32_t *list = nullptr;         // [cap] tree bodies (ascending), then the planes
    uint64_t *keys = nullptr, *keys_sorted = nullptr;          // [cap]
    uint32_t *parent = nullptr, *left = nullptr, *right = nullptr, *visit = nullptr, *rope = nullptr;   // [2 cap]
    float4 *nmin = nullptr, *nmax = nullptr;                   // [2 cap] node records: (min, left child | leaf body), (max, rope)
    Counters *cnt = nullptr;          // Morton bounds of this tree
    uint32_t *mask = nullptr;         // [cap / 32 + 1] ignore bits of the current call
    float4 *stage = nullptr;          // host entry point: p0 [kChunk], p1 [kChunk], out [2 kChunk]
    std::vector<void *> allocs;
    std::vector<uint32_t> host_list, host_mask;
    std::vector<float4> host_pts;
};

int query_tree_prepare(edynhip_ctx *c);   // raycast.hip: buffers on first use, boxes and tree when the state moved on

// ---- what the ticketed queries (query_async.hip) ask of raycast.hip and query_aabb.hip: the same kernels on a ticket's own buffers,
// everything enqueued on the context's stream, no host synchronisation on the steady path.
int ticket_trace(edynhip_ctx *c, uint32_t n, const float4 *p0, const float4 *p1, const uint32_t *ign_off, const uint32_t *ign_ids, uint32_t flags, uint4 *out);
// A box ticket's device buffers. Categories k = 0 .. 2 (EDYNHIP_QUERY_*) run the kernels of edynhip_query_aabb on arrays laid out by
// category: boxes_k[k][2 n] (a box that does not want category k holds NaN there and reports nothing), cnt_k / off_k[k][n],
// mid / big[k][n], ctl[k][2]. The caller's result is laid out by box: cnt4 / off4[4 i + k], k = 3 the of-interest list.
struct QaTicket {
    uint32_t n = 0, flags = 0, want_any = 0, capacity = 0;
    const float4 *boxes_k = nullptr;
    uint32_t *cnt_k = nullptr, *off_k = nullptr, *mid = nullptr, *big = nullptr, *ctl = nullptr;
    uint32_t *cnt4 = nullptr, *off4 = nullptr, *ids = nullptr;
    unsigned long long *tot = nullptr;
};
int ticket_query_count(edynhip_ctx *c, const QaTicket &t);   // tree, island boxes, and the counts of categories 0 .. 2 into cnt_k
int ticket_query_scan(edynhip_ctx *c, const QaTicket &t);    // off4[4 n + 1] and *tot from cnt4[4 n]
int ticket_query_fill(edynhip_ctx *c, const QaTicket &t);    // the lists of categories 0 .. 2 at off_k into ids[capacity]
// the island boxes the islands category tests (prepared by ticket_query_count when a box wants islands or of-interest lists):
// island label l exists iff flag[l], its box is (imin, imax)[slot[l]]; label[b]: the island of body b (a label beyond the bodies: b itself)
struct IslandView { const uint32_t *label, *flag, *slot; const float4 *imin, *imax; };
IslandView ticket_island_view(edynhip_ctx *c);

}  // namespace eh
