// Queries on a multi-device world: the kernels that turn the shards' answers into the answer of ONE context holding the whole scene.
// Every body is answered by exactly one shard (ctx.hpp edynhip_ctx::answers), with the single context's kernels and the same inputs, so
// a shard's hit record / hit list is bit for bit the single context's restricted to the shard's bodies. What is left:
//   - local body indices become global ones (k_world_translate_*; local_ids ascends, so order is kept);
//   - raycast: the single context keeps the smallest (fraction, body index) over all candidates, a minimum that does not depend on
//     the order of the candidates - k_world_rc_merge takes it over the shards' winners with raycast.hip rc_candidate's comparison;
//   - AABB: a query's hits are the union of the shards' ascending, pairwise disjoint lists. Offsets are the exclusive scan of the
//     summed counts (64-bit, stored saturated, as query_aabb.hip k_qa_scan); k_world_qa_merge places every hit at its query's offset
//     + its rank in its own list + the number of smaller ids in every other shard's list (binary searches): ascending without a sort.
#include "world_query.hpp"
#include <cfloat>

namespace eh {

constexpr uint32_t kWqNoBody = 0xFFFFFFFFu;
constexpr uint32_t kWqSat = 0xFFFFFFFFu;

__global__ void __launch_bounds__(256) k_world_translate_hits(uint32_t n, uint4 *__restrict__ hits, const uint32_t *__restrict__ local_ids, uint32_t n_local) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    uint32_t *body = (uint32_t *)&hits[2 * (size_t)r];
    const uint32_t b = *body;
    if (b < n_local) *body = local_ids[b];
}

__global__ void __launch_bounds__(256) k_world_translate_ids(size_t count, uint32_t *__restrict__ ids, const uint32_t *__restrict__ local_ids, uint32_t n_local) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t b = ids[i];
    if (b < n_local) ids[i] = local_ids[b];
}

// One lane per ray: the smallest (fraction, global body) of the shards' records, from a miss; the winner's 32 bytes unchanged.
__global__ void __launch_bounds__(256) k_world_rc_merge(uint32_t W, uint32_t n, const uint4 *__restrict__ hits, size_t stride, uint4 *__restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    uint4 b0 = make_uint4(kWqNoBody, __float_as_uint(FLT_MAX), 0u, 0u), b1 = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t s = 0; s < W; ++s) {
        const uint4 h0 = hits[s * stride + 2 * (size_t)r];
        const float f = __uint_as_float(h0.y), bf = __uint_as_float(b0.y);
        if (f < bf || (f == bf && b0.x != kWqNoBody && h0.x < b0.x)) { b0 = h0; b1 = hits[s * stride + 2 * (size_t)r + 1]; }
    }
    out[2 * (size_t)r] = b0;
    out[2 * (size_t)r + 1] = b1;
}

// inclusive scan over the workgroup (up to 1024 threads); `sh` holds one word per wave
__device__ __forceinline__ unsigned long long wq_block_scan(unsigned long long v, unsigned long long *sh, unsigned long long &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = (blockDim.x + 63u) >> 6;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    __syncthreads();   // (sh may still be read from the previous use)
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (uint32_t w = 0; w < nw; ++w) { const unsigned long long s = sh[w]; if (w < wave) before += s; all += s; }
    total = all;
    return v + before;
}
__device__ __forceinline__ uint32_t wq_sat(unsigned long long v) { return v >= kWqSat ? kWqSat : (uint32_t)v; }

// per query the sum of the shards' counts (disjoint bodies: at most the number of bodies, fits 32 bits), and the sums of 256 of them
__global__ void __launch_bounds__(256) k_world_qa_bsum(WqShards sh, uint32_t n, uint32_t *__restrict__ cnt_sum, unsigned long long *__restrict__ bsum) {
    __shared__ unsigned long long lds[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v = 0;
    if (i < n) {
        for (uint32_t s = 0; s < sh.W; ++s) v += sh.cnt[s][i];
        cnt_sum[i] = v;
    }
    unsigned long long total;
    (void)wq_block_scan(v, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ void __launch_bounds__(1024) k_world_qa_scan(uint32_t nb, const unsigned long long *__restrict__ bsum, unsigned long long *__restrict__ boff,
                                                        unsigned long long *tot64, uint32_t *end32, uint32_t *total32) {
    __shared__ unsigned long long lds[16];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < nb ? bsum[i] : 0ull;
        unsigned long long total;
        const unsigned long long incl = wq_block_scan(v, lds, total);
        if (i < nb) boff[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) { *tot64 = carry; *end32 = wq_sat(carry); *total32 = wq_sat(carry); }
}
__global__ void __launch_bounds__(256) k_world_qa_offsets(uint32_t n, const uint32_t *__restrict__ cnt_sum, const unsigned long long *__restrict__ boff,
                                                          uint32_t *__restrict__ out) {
    __shared__ unsigned long long lds[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = i < n ? cnt_sum[i] : 0u;
    unsigned long long total;
    const unsigned long long incl = wq_block_scan(v, lds, total);
    if (i < n) out[i] = wq_sat(boff[blockIdx.x] + incl - v);
}

// One lane per hit of shard `me`. Nothing is written at or beyond `capacity`.
__global__ void __launch_bounds__(256) k_world_qa_merge(WqShards sh, uint32_t me, uint32_t n, uint32_t num_hits, const uint32_t *__restrict__ offsets,
                                                        uint32_t *__restrict__ ids, uint32_t capacity) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_hits) return;
    const uint32_t *off = sh.off[me];
    uint32_t lo = 0, hi = n;   // the first index in [0, n] whose offset exceeds i (off[n] = num_hits > i); the query is the one before it
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] > i) hi = mid; else lo = mid + 1;
    }
    const uint32_t q = lo - 1;   // (off[0] = 0 <= i: lo >= 1)
    const uint32_t id = sh.ids[me][i];
    unsigned long long dst = (unsigned long long)offsets[q] + (i - off[q]);   // (a saturated offset is beyond every capacity)
    for (uint32_t s = 0; s < sh.W; ++s) {
        if (s == me) continue;
        const uint32_t b = sh.off[s][q], e = sh.off[s][q + 1];
        const uint32_t *seg = sh.ids[s];
        uint32_t l = b, h = e;   // lower bound of id in seg[b, e)
        while (l < h) {
            const uint32_t mid = l + ((h - l) >> 1);
            if (seg[mid] < id) l = mid + 1; else h = mid;
        }
        dst += l - b;
    }
    if (dst < capacity) ids[dst] = id;
}

static inline uint32_t wq_blocks(size_t n, uint32_t bs) { return (uint32_t)((n + bs - 1) / bs); }

void wq_translate_hits(hipStream_t s, uint32_t n, void *hits, const uint32_t *local_ids, uint32_t n_local) {
    if (n) hipLaunchKernelGGL(k_world_translate_hits, dim3(wq_blocks(n, 256)), dim3(256), 0, s, n, (uint4 *)hits, local_ids, n_local);
}
void wq_translate_ids(hipStream_t s, uint32_t *ids, size_t count, const uint32_t *local_ids, uint32_t n_local) {
    if (count) hipLaunchKernelGGL(k_world_translate_ids, dim3(wq_blocks(count, 256)), dim3(256), 0, s, count, ids, local_ids, n_local);
}
void wq_rc_merge(hipStream_t s, uint32_t W, uint32_t n, const void *shard_hits, size_t stride_hits, void *out) {
    if (n) hipLaunchKernelGGL(k_world_rc_merge, dim3(wq_blocks(n, 256)), dim3(256), 0, s, W, n, (const uint4 *)shard_hits, 2 * stride_hits, (uint4 *)out);
}
void wq_qa_offsets(hipStream_t s, const WqShards &sh, uint32_t n, uint32_t *cnt_sum, unsigned long long *bsum, unsigned long long *boff,
                   unsigned long long *tot64, uint32_t *offsets, uint32_t *total) {
    const uint32_t nb = wq_blocks(n, 256);
    if (nb) hipLaunchKernelGGL(k_world_qa_bsum, dim3(nb), dim3(256), 0, s, sh, n, cnt_sum, bsum);
    hipLaunchKernelGGL(k_world_qa_scan, dim3(1), dim3(1024), 0, s, nb, bsum, boff, tot64, offsets + n, total);
    if (nb) hipLaunchKernelGGL(k_world_qa_offsets, dim3(nb), dim3(256), 0, s, n, cnt_sum, boff, offsets);
}
void wq_qa_merge(hipStream_t s, const WqShards &sh, uint32_t shard, uint32_t n, uint32_t num_hits, const uint32_t *offsets, uint32_t *ids, uint32_t capacity) {
    if (num_hits && n) hipLaunchKernelGGL(k_world_qa_merge, dim3(wq_blocks(num_hits, 256)), dim3(256), 0, s, sh, shard, n, num_hits, offsets, ids, capacity);
}

}  // namespace eh
