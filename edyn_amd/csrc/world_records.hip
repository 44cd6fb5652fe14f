// Record hand-over of a multi-device world (multi_records.hip edynhip_world_snapshot_records / edynhip_world_snapshot_map): what a shard context
// does for it. Every shard packs the 96-byte registry records (edynhip_body_record) of the bodies it reports - its own dynamic bodies,
// shard 0 also the replicated ones: the context's `answers` bits - with the single context's record arithmetic (drecord.hpp body_record)
// and stores them at the bodies' GLOBAL indices straight into the world's pinned slot, which is mapped into every shard's device. No
// staging buffer, no host scatter; 16-byte vector stores only, no LDS, no atomics.
//
// Lane mapping (kRecordLanes, a build-time choice). 1 (the default): one lane per record - six float4 stores per lane, neighbouring lanes
// 96 bytes apart, the mapping of the single context's k_pack_records. 6: six lanes per record, each storing one float4 - a record leaves
// as one 96-byte burst and a wave instruction covers ten whole records back to back where the global indices are consecutive (they
// ascend with the local ones); the six lanes evaluate the record redundantly (their loads hit the same lines). Measured on pile32k, two
// shards on one GPU (scripts/bench_world_records.py): no difference beyond the run-to-run spread, so the plainer
// mapping stays; the other one is kept behind the macro for a box where a second device stores into the slot, which nobody has measured.
#include "ctx.hpp"
#include "drecord.hpp"

#ifndef EDYNHIP_WORLD_RECORD_LANES
#define EDYNHIP_WORLD_RECORD_LANES 1
#endif

namespace eh {

constexpr int kRecordLanes = EDYNHIP_WORLD_RECORD_LANES;
static_assert(kRecordLanes == 1 || kRecordLanes == 6, "one lane per record, or one lane per float4 of a record");

template <int LANES>
__global__ void __launch_bounds__(LANES == 1 ? 256 : 192) k_world_pack_records(uint32_t n_local, Bodies b, const uint32_t *__restrict__ answers,
                                                                               const uint32_t *__restrict__ local_ids, uint32_t num_bodies,
                                                                               float present_dt, float4 *__restrict__ dst) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t l = t / LANES, part = t % LANES;
    if (l >= n_local) return;
    if (answers && !((answers[l >> 5] >> (l & 31u)) & 1u)) return;   // another shard reports this (replicated) body
    const uint32_t g = local_ids[l];
    if (g >= num_bodies) return;                                      // (the slot holds num_bodies records)
    float4 rec[6];
    body_record(b, l, present_dt, rec);
    float4 *o = dst + (size_t)g * 6;
    if (LANES == 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = rec[k];
    } else {
        float4 v = rec[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) if (part == (uint32_t)k) v = rec[k];
        o[part] = v;
    }
}

int shard_pack_records(edynhip_ctx *c, const uint32_t *local_ids_dev, uint32_t n_local, uint32_t num_bodies, float present_dt, void *records) {
    if (n_local == 0) return EDYNHIP_OK;
    if (n_local > c->b.n) return set_error(c, EDYNHIP_ERR_INTERNAL, "shard_pack_records: more local bodies than the context holds");
    constexpr uint32_t bs = kRecordLanes == 1 ? 256u : 192u;
    const uint64_t threads = (uint64_t)n_local * kRecordLanes;
    hipLaunchKernelGGL(k_world_pack_records<kRecordLanes>, dim3((uint32_t)((threads + bs - 1) / bs)), dim3(bs), 0, c->stream, n_local, c->b, c->answers,
                       local_ids_dev, num_bodies, present_dt, (float4 *)records);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

}  // namespace eh
