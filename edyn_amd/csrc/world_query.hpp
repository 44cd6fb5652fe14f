// Queries on a multi-device world (multi_query.hip edynhip_world_raycast / edynhip_world_query_aabb): what runs beside the shards' own
// kernels - index translation on a shard's device, and the merges on the world's home device (world_query.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace eh {

constexpr uint32_t kWorldMaxShards = 64;   // edynhip_world_create's limit

// the shards' answers to one batch of boxes, on the home device: counts [n], offsets [n + 1] and ascending GLOBAL ids per shard
struct WqShards {
    uint32_t W;
    const uint32_t *cnt[kWorldMaxShards], *off[kWorldMaxShards], *ids[kWorldMaxShards];
};

// on a shard's device: local body indices -> global ones (indices beyond n_local, the miss's ~0u among them, stay)
void wq_translate_hits(hipStream_t s, uint32_t n, void *hits, const uint32_t *local_ids, uint32_t n_local);
void wq_translate_ids(hipStream_t s, uint32_t *ids, size_t count, const uint32_t *local_ids, uint32_t n_local);
// on the home device
void wq_rc_merge(hipStream_t s, uint32_t W, uint32_t n, const void *shard_hits, size_t stride_hits, void *out);
// cnt_sum [n], bsum / boff [n / 256 + 2], tot64 [1]: scratch; offsets [n + 1] and total [1] are the caller's
void wq_qa_offsets(hipStream_t s, const WqShards &sh, uint32_t n, uint32_t *cnt_sum, unsigned long long *bsum, unsigned long long *boff,
                   unsigned long long *tot64, uint32_t *offsets, uint32_t *total);
void wq_qa_merge(hipStream_t s, const WqShards &sh, uint32_t shard, uint32_t n, uint32_t num_hits, const uint32_t *offsets, uint32_t *ids, uint32_t capacity);

}  // namespace eh
