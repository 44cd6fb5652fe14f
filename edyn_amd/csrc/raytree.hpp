// The query tree the raycast (raycast.hip) and the AABB queries (query_aabb.hip) share: per-body boxes from the current transforms and a
// linear BVH with ropes over every shaped non-plane body, rebuilt by query_tree_prepare at the first query after
// edynhip_ctx::state_epoch moved on. Leaves hold exactly (AABB - 0.1, AABB + 0.1), internal nodes a superset of their children.
#pragma once
#include "ctx.hpp"
#include <vector>

namespace eh {

constexpr float kFatInset = 0.1f;             // dynamic_tree::aabb_inset = -0.1 (dynamic_tree.hpp:24, dynamic_tree.cpp:45)
constexpr uint32_t kLeafBit = 0x80000000u;    // nmin.w of a leaf: kLeafBit | body; of an internal node: its left child
constexpr uint32_t kRayEnd = 0xFFFFFFFFu;     // rope of the last node of a depth-first walk (broadphase.hip kRopeEnd)

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

}  // namespace eh
