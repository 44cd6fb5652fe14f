// AABB queries (edyn::query_procedural_aabb / query_non_procedural_aabb / query_island_aabb, include/edyn/collision/query_aabb.hpp:10-26,
// broadphase.hpp:81-100, dynamic_tree.cpp query) for batches of boxes, answered on the device with a variable-length (CSR) result.
// The reference asks its three trees; a leaf is reported iff intersect_aabb(query, leaf box) (geom.cpp:762-770), where a freshly created
// leaf holds the AABB grown by 0.1 (dynamic_tree.hpp:24). Here the raycast's query tree (raytree.hpp) is walked with the box: its leaves
// hold exactly that box and its internal nodes a superset of their children, and each of the six comparisons is monotone in the node
// box, so the same six comparisons on an internal node never skip a passing leaf - also for inverted queries, which are not special.
//   Two passes over the queries: k_qa_count (one lane per query counts its hits), an exclusive scan of the counts (k_qa_bsum,
// k_qa_scan, k_qa_offsets: 64-bit sums, stored saturated to 32 bits), and the fill. Hits are reported in ascending body index:
//   - up to kLaneSort hits: the query's lane writes them in tree order and sorts its segment in place (k_qa_fill);
//   - up to kSortMax hits: the lane writes them, then one wave sorts the segment in LDS (k_qa_sort);
//   - more than kSortMax hits, or more than 1 / 64 of all bodies (kScanRatioDefault): one wave strides the body range with the exact predicate and
//     packs with ballot + prefix, ascending by construction (k_qa_scan_fill).
// Brute force (test aid) and the island category loop over every body / island in ascending order with the same predicate.
#include "ctx.hpp"
#include "dmath.hpp"
#include "raytree.hpp"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace eh {
using namespace dm;

constexpr uint32_t kQaChunk = 1u << 20;      // queries per launch
constexpr uint32_t kLaneSort = 32;           // segments up to this many hits are sorted by the lane that wrote them
constexpr uint32_t kSortMax = 4096;          // segments up to this many hits are sorted by one wave in LDS
// A query that reports more than n_bodies / ratio bodies strides the body range instead. 64 was measured on ONE scene (the settled
// headline pile, 32 769 bodies: DESIGN §8 "AABB queries"). The stride costs n_bodies / 64 wave iterations per query whatever the
// count, and kSortMax caps the lane path at 4096 hits, so on 262k - 1M bodies a 4097-hit query takes 4k - 16k iterations: whether
// that still beats the lane path there is unmeasured (striding the leaves of the query's subtree would scale with the count instead).
constexpr uint32_t kScanRatioDefault = 64;
constexpr uint32_t kSat = 0xFFFFFFFFu;       // a 32-bit offset / total that does not fit
enum { QA_TREE = 0, QA_BRUTE = 1, QA_ISLANDS = 2 };

struct QueryAabb {
    uint32_t n_cap = 0;               // queries the per-query buffers hold
    uint32_t *cnt = nullptr;          // [n_cap] hits per query
    unsigned long long *bsum = nullptr, *boff = nullptr;   // [n_cap / 256 + 1] sums of 256 counts, their exclusive scan
    uint32_t *mid = nullptr, *big = nullptr;               // [n_cap] queries whose segment a wave sorts / a wave fills
    uint32_t *ctl = nullptr;          // [8]: 0 n_mid, 1 n_big (this call); 2 n_islands; 4.. statistics (unsigned long long x 2)
    unsigned long long *tot = nullptr;                      // [2] 64-bit total of the last scan (queries, islands)
    // islands: per label the union of the query tree's boxes of its shaped dynamic bodies, compacted in ascending label order
    uint32_t isl_cap = 0;
    uint64_t isl_epoch = 0;
    uint32_t *lo = nullptr, *hi = nullptr, *flag = nullptr, *slot = nullptr;   // [3 cap] ordered bits, [cap], [cap]
    float4 *imin = nullptr, *imax = nullptr;                                   // [cap] (min, label), (max, -)
    // host entry point: device copies of the caller's arrays (grown on demand)
    float4 *d_boxes = nullptr; uint32_t *d_off = nullptr, *d_ids = nullptr, *d_total = nullptr;
    size_t boxes_cap = 0, off_cap = 0, ids_cap = 0;
    std::vector<float4> host_boxes, stage_boxes;   // the boxes on the device, and the ones of the current call
    // the host entry point's last count pass: a following call with the same boxes on the same state (the caller asking again with an
    // ids buffer sized by the total) keeps its counts, offsets and lists instead of walking the tree again
    bool counted = false;
    uint64_t counted_epoch = 0;
    int counted_category = 0;
    uint32_t counted_flags = 0, counted_n = 0;
    unsigned long long counted_total = 0;
    uint32_t scan_ratio = kScanRatioDefault;
};

void query_aabb_free(edynhip_ctx *c) {
    if (!c->qa) return;
    QueryAabb &q = *c->qa;
    void *all[] = {q.cnt, q.bsum, q.boff, q.mid, q.big, q.ctl, q.tot, q.lo, q.hi, q.flag, q.slot, q.imin, q.imax, q.d_boxes, q.d_off, q.d_ids, q.d_total};
    for (void *p : all) if (p) (void)hipFree(p);
    delete c->qa;
    c->qa = nullptr;
}

template <typename T>
static int qalloc(edynhip_ctx *c, T *&p, size_t count) {
    if (p) { (void)hipFree(p); p = nullptr; }
    void *q = nullptr;
    EH_HIP(c, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    p = (T *)q;
    return EDYNHIP_OK;
}

struct QaArgs {
    const uint32_t *flags;
    const float4 *amin, *amax;        // the query tree's per-body boxes
    const float4 *nmin, *nmax;
    uint32_t n_tree;
    const uint32_t *planes;
    uint32_t n_planes, n_bodies;
    const float4 *imin, *imax;        // islands
    const uint32_t *n_islands;
    const uint32_t *answers;          // a shard of a multi-device world: bit per body it answers for; nullptr: every body
    uint32_t category, mode, scan_ratio;
};

// (qa_overlap, qa_fat_min, qa_fat_max: raytree.hpp - the of-interest pass of query_async.hip runs the same test)
// procedural: shaped, not removed, dynamic (capi.hip rebuild_broadphase_lists); non-procedural: shaped, not removed, static or kinematic
DI bool qa_category(const QaArgs &a, uint32_t body) {
    if (a.answers && !((a.answers[body >> 5] >> (body & 31u)) & 1u)) return false;   // another shard's to answer
    const uint32_t fl = a.flags[body];
    if ((fl & BF_SHAPE_MASK) == 0 || (fl & BF_REMOVED)) return false;
    const bool dyn = (fl & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC;
    return dyn == (a.category == EDYNHIP_QUERY_PROCEDURAL);
}
DI bool qa_body(const QaArgs &a, uint32_t body, f3 qmn, f3 qmx) {
    return qa_category(a, body) && qa_overlap(qmn, qmx, qa_fat_min(a.amin[body]), qa_fat_max(a.amax[body]));
}
// which fill path a query of the tree walk takes: 0 lane (sorted by the lane), 1 lane + wave sort, 2 wave over the body range
DI int qa_tier(const QaArgs &a, uint32_t count) {
    if (a.mode != QA_TREE || count <= kLaneSort) return 0;
    if (count > kSortMax || (unsigned long long)count * a.scan_ratio > a.n_bodies) return 2;
    return 1;
}

template <typename F>
DI void qa_walk(const QaArgs &a, f3 qmn, f3 qmx, F &&emit) {
    if (a.mode == QA_BRUTE) {
        for (uint32_t b = 0; b < a.n_bodies; ++b)
            if (qa_body(a, b, qmn, qmx)) emit(b);
    } else if (a.mode == QA_ISLANDS) {
        const uint32_t ni = *a.n_islands;
        for (uint32_t k = 0; k < ni; ++k) {
            const float4 lo = a.imin[k], hi = a.imax[k];
            if (qa_overlap(qmn, qmx, qa_fat_min(lo), qa_fat_max(hi))) emit(__float_as_uint(lo.w));
        }
    } else {
        if (a.category == EDYNHIP_QUERY_NON_PROCEDURAL)
            for (uint32_t k = 0; k < a.n_planes; ++k) {
                const uint32_t b = a.planes[k];
                if (qa_body(a, b, qmn, qmx)) emit(b);
            }
        uint32_t node = a.n_tree ? 0u : kRayEnd;   // the root: internal node 0, or leaf 0 of a one-body tree
        while (node != kRayEnd) {
            const float4 lo = a.nmin[node], hi = a.nmax[node];
            const uint32_t w = __float_as_uint(lo.w);
            const bool over = qa_overlap(qmn, qmx, mk3(lo.x, lo.y, lo.z), mk3(hi.x, hi.y, hi.z));
            if (w & kLeafBit) {   // the leaf's box is the body's own (AABB - 0.1, AABB + 0.1): the exact predicate
                if (over && qa_category(a, w & ~kLeafBit)) emit(w & ~kLeafBit);
                node = __float_as_uint(hi.w);
            } else {
                node = over ? w : __float_as_uint(hi.w);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_qa_count(QaArgs a, uint32_t n, const float4 *__restrict__ boxes, uint32_t first, uint32_t want_ids,
                                                  uint32_t *__restrict__ cnt, uint32_t *__restrict__ mid, uint32_t *__restrict__ big, uint32_t *ctl) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t count = 0;
    if (q < n) {
        const f3 qmn = from4(boxes[2 * (size_t)q]), qmx = from4(boxes[2 * (size_t)q + 1]);
        qa_walk(a, qmn, qmx, [&](uint32_t) { ++count; });
        cnt[q] = count;
    }
    if (!want_ids) return;
    // the lists of the two wave paths: one atomic per wave and list (ballot, the first listed lane reserves the slots)
    const int tier = q < n ? qa_tier(a, count) : 0;
    const uint32_t lane = threadIdx.x & 63u;
    for (int t = 1; t <= 2; ++t) {
        const unsigned long long m = __ballot(tier == t);
        if (m == 0) continue;   // (wave-uniform)
        const int leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(&ctl[t - 1], (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (tier == t) (t == 1 ? mid : big)[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = first + q;
    }
}

// inclusive scan over the workgroup (up to 1024 threads); `sh` holds one word per wave
DI unsigned long long qa_block_scan(unsigned long long v, unsigned long long *sh, unsigned long long &total) {
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

__global__ void __launch_bounds__(256) k_qa_bsum(uint32_t n, const uint32_t *__restrict__ cnt, unsigned long long *__restrict__ bsum) {
    __shared__ unsigned long long sh[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long total;
    (void)qa_block_scan(i < n ? cnt[i] : 0u, sh, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

DI uint32_t qa_sat(unsigned long long v) { return v >= kSat ? kSat : (uint32_t)v; }

// one workgroup: exclusive scan of the block sums, the 64-bit total, and its saturated copies (offsets[n], the caller's total)
__global__ void __launch_bounds__(1024) k_qa_scan(uint32_t nb, const unsigned long long *__restrict__ bsum, unsigned long long *__restrict__ boff,
                                                  unsigned long long *tot64, uint32_t *end32, uint32_t *total32) {
    __shared__ unsigned long long sh[16];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < nb ? bsum[i] : 0ull;
        unsigned long long total;
        const unsigned long long incl = qa_block_scan(v, sh, total);
        if (i < nb) boff[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) {
        *tot64 = carry;
        if (end32) *end32 = qa_sat(carry);
        if (total32) *total32 = qa_sat(carry);
    }
}

__global__ void __launch_bounds__(256) k_qa_offsets(uint32_t n, const uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ boff,
                                                    uint32_t *__restrict__ out) {
    __shared__ unsigned long long sh[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = i < n ? cnt[i] : 0u;
    unsigned long long total;
    const unsigned long long incl = qa_block_scan(v, sh, total);
    if (i < n) out[i] = qa_sat(boff[blockIdx.x] + incl - v);
}

// The lane path: hits written at the query's offset (nothing at or beyond `capacity`); short segments sorted in place.
__global__ void __launch_bounds__(256) k_qa_fill(QaArgs a, uint32_t n, const float4 *__restrict__ boxes, const uint32_t *__restrict__ cnt,
                                                 const uint32_t *__restrict__ offsets, uint32_t *__restrict__ ids, uint32_t capacity) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint32_t count = cnt[q], start = offsets[q];
    if (count == 0 || start == kSat || start >= capacity || qa_tier(a, count) == 2) return;
    const f3 qmn = from4(boxes[2 * (size_t)q]), qmx = from4(boxes[2 * (size_t)q + 1]);
    const uint32_t room = capacity - start;
    uint32_t *seg = ids + start;
    uint32_t k = 0;
    qa_walk(a, qmn, qmx, [&](uint32_t id) { if (k < room) seg[k] = id; ++k; });
    if (a.mode != QA_TREE || count > kLaneSort || count > room) return;
    for (uint32_t i = 1; i < count; ++i) {
        const uint32_t v = seg[i];
        uint32_t j = i;
        while (j > 0 && seg[j - 1] > v) { seg[j] = seg[j - 1]; --j; }
        seg[j] = v;
    }
}

// One wave per listed query: bitonic sort of its segment (33 .. kSortMax ids) in LDS.
__global__ void __launch_bounds__(64) k_qa_sort(const uint32_t *__restrict__ list, const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ cnt,
                                                const uint32_t *__restrict__ offsets, uint32_t *__restrict__ ids, uint32_t capacity, unsigned long long *stats) {
    __shared__ uint32_t s[kSortMax];
    const uint32_t nl = ctl[0];
    uint32_t done = 0;
    for (uint32_t idx = blockIdx.x; idx < nl; idx += gridDim.x) {
        const uint32_t q = list[idx], count = cnt[q], start = offsets[q];
        if (start == kSat || start >= capacity || count > capacity - start || count > kSortMax) continue;   // (overflow: ids are unspecified)
        uint32_t P = 64;
        while (P < count) P <<= 1;
        for (uint32_t t = threadIdx.x; t < P; t += 64) s[t] = t < count ? ids[start + t] : 0xFFFFFFFFu;
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = threadIdx.x; t < P / 2; t += 64) {
                    const uint32_t i = 2 * t - (t & (j - 1)), l = i + j;
                    const uint32_t x = s[i], y = s[l];
                    if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
                }
                __syncthreads();
            }
        for (uint32_t t = threadIdx.x; t < count; t += 64) ids[start + t] = s[t];
        __syncthreads();
        ++done;
    }
    if (threadIdx.x == 0 && done) atomicAdd(stats, (unsigned long long)done);   // edynhip_query_aabb_stats: segments a wave sorted
}

// One wave per listed query: lanes stride the body range with the exact predicate; ballot + prefix pack in ascending body index.
__global__ void __launch_bounds__(256) k_qa_scan_fill(QaArgs a, const float4 *__restrict__ boxes, const uint32_t *__restrict__ list,
                                                      const uint32_t *__restrict__ ctl, const uint32_t *__restrict__ offsets,
                                                      uint32_t *__restrict__ ids, uint32_t capacity, unsigned long long *stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t nl = ctl[1];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t done = 0;
    for (uint32_t idx = wave; idx < nl; idx += nwaves) {
        const uint32_t q = list[idx], start = offsets[q];
        if (start == kSat || start >= capacity) continue;
        const f3 qmn = from4(boxes[2 * (size_t)q]), qmx = from4(boxes[2 * (size_t)q + 1]);
        unsigned long long pos = start;
        for (uint32_t base = 0; base < a.n_bodies; base += 64) {
            const uint32_t b = base + lane;
            const bool hit = b < a.n_bodies && qa_body(a, b, qmn, qmx);
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const unsigned long long at = pos + (unsigned long long)__popcll(m & below);
                if (at < capacity) ids[at] = b;
            }
            pos += (unsigned long long)__popcll(m);
        }
        ++done;
    }
    if (lane == 0 && done) atomicAdd(stats + 1, (unsigned long long)done);   // edynhip_query_aabb_stats: queries a wave packed
}

// ---- islands: segmented min / max of the query tree's per-body boxes by island label (multi_partition.hip k_island_box_* on Bodies::amin / amax)
DI uint32_t qa_ordered(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
DI float qa_unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
__global__ void k_qa_isl_clear(uint32_t n, uint32_t *lo, uint32_t *hi, uint32_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * n) { lo[i] = 0xFFFFFFFFu; hi[i] = 0u; }
    if (i < n) flag[i] = 0u;
}
__global__ void k_qa_isl_reduce(uint32_t n, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ island, const uint32_t *__restrict__ answers,
                                const float4 *__restrict__ amin, const float4 *__restrict__ amax, uint32_t *lo, uint32_t *hi, uint32_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (answers && !((answers[i >> 5] >> (i & 31u)) & 1u)) return;
    const uint32_t fl = flags[i];
    if ((fl & BF_KIND_MASK) != EDYNHIP_KIND_DYNAMIC || (fl & BF_REMOVED) || (fl & BF_SHAPE_MASK) == 0) return;
    uint32_t l = island[i];
    if (l >= n) l = i;
    const float4 mn = amin[i], mx = amax[i];
    atomicMin(&lo[3 * l], qa_ordered(mn.x)); atomicMin(&lo[3 * l + 1], qa_ordered(mn.y)); atomicMin(&lo[3 * l + 2], qa_ordered(mn.z));
    atomicMax(&hi[3 * l], qa_ordered(mx.x)); atomicMax(&hi[3 * l + 1], qa_ordered(mx.y)); atomicMax(&hi[3 * l + 2], qa_ordered(mx.z));
    flag[l] = 1u;
}
__global__ void k_qa_isl_compact(uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ slot, const uint32_t *__restrict__ lo,
                                 const uint32_t *__restrict__ hi, float4 *__restrict__ imin, float4 *__restrict__ imax) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n || !flag[l]) return;
    const uint32_t k = slot[l];   // (< n: at most one island per body)
    imin[k] = make_float4(qa_unordered(lo[3 * l]), qa_unordered(lo[3 * l + 1]), qa_unordered(lo[3 * l + 2]), __uint_as_float(l));
    imax[k] = make_float4(qa_unordered(hi[3 * l]), qa_unordered(hi[3 * l + 1]), qa_unordered(hi[3 * l + 2]), 0.0f);
}

static inline uint32_t nblocks(uint32_t n, uint32_t bs) { return (n + bs - 1) / bs; }

// exclusive scan of cnt[n] into out[n]; the 64-bit total to *tot64, saturated to *end32 / *total32 (either may be null)
static int scan_counts(edynhip_ctx *c, QueryAabb &q, uint32_t n, const uint32_t *cnt, uint32_t *out, unsigned long long *tot64, uint32_t *end32, uint32_t *total32) {
    const uint32_t nb = nblocks(n, 256);
    if (nb) hipLaunchKernelGGL(k_qa_bsum, dim3(nb), dim3(256), 0, c->stream, n, cnt, q.bsum);
    hipLaunchKernelGGL(k_qa_scan, dim3(1), dim3(1024), 0, c->stream, nb, q.bsum, q.boff, tot64, end32, total32);
    if (nb) hipLaunchKernelGGL(k_qa_offsets, dim3(nb), dim3(256), 0, c->stream, n, cnt, q.boff, out);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

// buffers for n queries (and, for the island category, for the context's body capacity)
static int qa_reserve(edynhip_ctx *c, uint32_t n, bool islands) {
    if (!c->qa) {
        c->qa = new QueryAabb();
        { const long v = c->knobs.query_scan_ratio; if (v > 0 && v < (1 << 20)) c->qa->scan_ratio = (uint32_t)v; }   // developer knob EDYNHIP_QUERY_SCAN_RATIO
    }
    QueryAabb &q = *c->qa;
    if (!q.ctl) {
        EH_TRY(qalloc(c, q.ctl, 8)); EH_TRY(qalloc(c, q.tot, 2));
        EH_HIP(c, hipMemsetAsync(q.ctl, 0, 8 * sizeof(uint32_t), c->stream));
    }
    const uint32_t need = std::max(n, islands ? c->b.cap : 0u);
    if (need > q.n_cap) {
        EH_HIP(c, hipStreamSynchronize(c->stream));   // (earlier queries on the stream may still use the old buffers)
        const uint32_t cap = std::max(need, 1024u);
        q.n_cap = 0; q.counted = false;   // (a failed growth leaves no capacity behind: the next call allocates again)
        EH_TRY(qalloc(c, q.cnt, cap)); EH_TRY(qalloc(c, q.mid, cap)); EH_TRY(qalloc(c, q.big, cap));
        EH_TRY(qalloc(c, q.bsum, cap / 256 + 2)); EH_TRY(qalloc(c, q.boff, cap / 256 + 2));
        q.n_cap = cap;
    }
    if (islands && q.isl_cap != c->b.cap) {
        EH_HIP(c, hipStreamSynchronize(c->stream));
        const uint32_t cap = c->b.cap;
        q.isl_cap = 0;
        EH_TRY(qalloc(c, q.lo, 3 * (size_t)cap)); EH_TRY(qalloc(c, q.hi, 3 * (size_t)cap)); EH_TRY(qalloc(c, q.flag, cap)); EH_TRY(qalloc(c, q.slot, cap));
        EH_TRY(qalloc(c, q.imin, cap)); EH_TRY(qalloc(c, q.imax, cap));
        q.isl_cap = cap; q.isl_epoch = 0;
    }
    return EDYNHIP_OK;
}

static int prepare_islands(edynhip_ctx *c) {
    QueryAabb &q = *c->qa;
    if (q.isl_epoch == c->state_epoch) return EDYNHIP_OK;
    const RayTree &t = *c->ray;
    const uint32_t n = c->b.n;
    if (n) {
        hipLaunchKernelGGL(k_qa_isl_clear, dim3(nblocks(3 * n, 256)), dim3(256), 0, c->stream, n, q.lo, q.hi, q.flag);
        hipLaunchKernelGGL(k_qa_isl_reduce, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->b.flags,
                           c->query_island && c->step_index == 0 ? c->query_island : c->b.island, c->answers, t.amin, t.amax, q.lo, q.hi, q.flag);
    }
    EH_TRY(scan_counts(c, q, n, q.flag, q.slot, q.tot + 1, q.ctl + 2, nullptr));
    if (n) hipLaunchKernelGGL(k_qa_isl_compact, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, q.flag, q.slot, q.lo, q.hi, q.imin, q.imax);
    EH_HIP(c, hipGetLastError());
    q.isl_epoch = c->state_epoch;
    return EDYNHIP_OK;
}

// Everything on the context's stream, no host synchronisation: offsets[n + 1] and *total always, ids (when given) up to capacity.
static int run_query(edynhip_ctx *c, int category, uint32_t n, const float4 *boxes, uint32_t flags, uint32_t *offsets, uint32_t *ids, uint32_t capacity,
                     uint32_t *total, bool classify = false, bool counted = false) {
    const bool islands = category == EDYNHIP_QUERY_ISLANDS;
    EH_TRY(query_tree_prepare(c));
    EH_TRY(qa_reserve(c, n, islands));
    if (islands) { EH_TRY(prepare_islands(c)); }
    QueryAabb &q = *c->qa;
    const RayTree &t = *c->ray;
    QaArgs a;
    a.flags = c->b.flags; a.amin = t.amin; a.amax = t.amax; a.nmin = t.nmin; a.nmax = t.nmax; a.n_tree = t.n_tree;
    a.planes = t.list + t.n_tree; a.n_planes = t.n_planes; a.n_bodies = c->b.n;
    a.imin = q.imin; a.imax = q.imax; a.n_islands = q.ctl + 2; a.answers = c->answers;
    a.category = (uint32_t)category; a.scan_ratio = q.scan_ratio;
    a.mode = islands ? QA_ISLANDS : (flags & EDYNHIP_QUERY_BRUTE_FORCE) ? QA_BRUTE : QA_TREE;
    const uint32_t want_ids = ids && capacity ? 1u : 0u;
    if (!counted) {   // (the host entry point's second call keeps the counts, offsets and lists of its first)
        q.counted = false;
        EH_HIP(c, hipMemsetAsync(q.ctl, 0, 2 * sizeof(uint32_t), c->stream));
        for (uint32_t off = 0; off < n; off += kQaChunk) {
            const uint32_t m = std::min(kQaChunk, n - off);
            hipLaunchKernelGGL(k_qa_count, dim3(nblocks(m, 256)), dim3(256), 0, c->stream, a, m, boxes + 2 * (size_t)off, off, want_ids | (classify ? 1u : 0u),
                               q.cnt + off, q.mid, q.big, q.ctl);
        }
        EH_TRY(scan_counts(c, q, n, q.cnt, offsets, q.tot, offsets + n, total));
    }
    if (!want_ids || n == 0) return EDYNHIP_OK;
    for (uint32_t off = 0; off < n; off += kQaChunk) {
        const uint32_t m = std::min(kQaChunk, n - off);
        hipLaunchKernelGGL(k_qa_fill, dim3(nblocks(m, 256)), dim3(256), 0, c->stream, a, m, boxes + 2 * (size_t)off, q.cnt + off, offsets + off, ids, capacity);
    }
    if (a.mode == QA_TREE) {   // (their lists may be empty: the kernels read the lengths on the device)
        hipLaunchKernelGGL(k_qa_sort, dim3(std::min(n, 2048u)), dim3(64), 0, c->stream, q.mid, q.ctl, q.cnt, offsets, ids, capacity, (unsigned long long *)(q.ctl + 4));
        hipLaunchKernelGGL(k_qa_scan_fill, dim3(std::min(nblocks(n, 4), 1024u)), dim3(256), 0, c->stream, a, boxes, q.big, q.ctl, offsets, ids, capacity, (unsigned long long *)(q.ctl + 4));
    }
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

// A world's count pass on this shard: counts, offsets and total stay in the context's buffers (the host entry point's), where the world reads them.
int shard_query_count(edynhip_ctx *c, int category, uint32_t n, const void *boxes_f4, uint32_t flags, const uint32_t **cnt, const uint32_t **offsets,
                      const unsigned long long **tot64) {
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(qa_reserve(c, n, false));
    QueryAabb &q = *c->qa;
    q.counted = false;
    if ((size_t)n + 1 > q.off_cap) {
        EH_HIP(c, hipStreamSynchronize(c->stream));
        q.off_cap = 0;
        EH_TRY(qalloc(c, q.d_off, (size_t)n + 1));
        q.off_cap = (size_t)n + 1;
    }
    if (!q.d_total) EH_TRY(qalloc(c, q.d_total, 1));
    EH_TRY(run_query(c, category, n, (const float4 *)boxes_f4, flags, q.d_off, nullptr, 0, q.d_total, true));
    c->qa->counted = false;   // (not the host entry point's boxes)
    *cnt = q.cnt; *offsets = q.d_off; *tot64 = q.tot;
    return EDYNHIP_OK;
}

int shard_query_fill(edynhip_ctx *c, int category, uint32_t n, const void *boxes_f4, uint32_t flags, uint32_t *ids, uint32_t capacity) {
    EH_HIP(c, hipSetDevice(c->device));
    QueryAabb &q = *c->qa;
    return run_query(c, category, n, (const float4 *)boxes_f4, flags, q.d_off, ids, capacity, q.d_total, false, true);
}

// ---- a box ticket (query_async.hip): the kernels above on the ticket's own buffers. Of the context's QueryAabb only what lives inside
// one enqueue (the scan's block sums) or is keyed by state_epoch (the island boxes) is used: not cnt, mid, big, ctl[0..1], d_* or the
// `counted` cache, which belong to the synchronous entry points.
static QaArgs ticket_args(edynhip_ctx *c, int category, uint32_t flags) {
    const QueryAabb &q = *c->qa;
    const RayTree &t = *c->ray;
    QaArgs a;
    a.flags = c->b.flags; a.amin = t.amin; a.amax = t.amax; a.nmin = t.nmin; a.nmax = t.nmax; a.n_tree = t.n_tree;
    a.planes = t.list + t.n_tree; a.n_planes = t.n_planes; a.n_bodies = c->b.n;
    a.imin = q.imin; a.imax = q.imax; a.n_islands = q.ctl + 2; a.answers = c->answers;
    a.category = (uint32_t)category; a.scan_ratio = q.scan_ratio;
    a.mode = category == EDYNHIP_QUERY_ISLANDS ? QA_ISLANDS : (flags & EDYNHIP_QUERY_BRUTE_FORCE) ? QA_BRUTE : QA_TREE;
    return a;
}
int ticket_query_count(edynhip_ctx *c, const QaTicket &t) {
    const bool islands = (t.want_any & (EDYNHIP_WANT_ISLANDS | EDYNHIP_WANT_OF_INTEREST)) != 0;
    EH_TRY(query_tree_prepare(c));
    EH_TRY(qa_reserve(c, 4 * t.n, islands));
    if (islands) { EH_TRY(prepare_islands(c)); }
    const uint32_t n = t.n;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipMemsetAsync(t.cnt_k, 0, 3 * (size_t)n * sizeof(uint32_t), c->stream));   // (a category nobody wants is not counted)
    EH_HIP(c, hipMemsetAsync(t.ctl, 0, 6 * sizeof(uint32_t), c->stream));
    for (int k = 0; k < 3; ++k) {
        if (!(t.want_any & (1u << k))) continue;
        const QaArgs a = ticket_args(c, k, t.flags);
        for (uint32_t off = 0; off < n; off += kQaChunk) {
            const uint32_t m = std::min(kQaChunk, n - off);
            hipLaunchKernelGGL(k_qa_count, dim3(nblocks(m, 256)), dim3(256), 0, c->stream, a, m, t.boxes_k + 2 * ((size_t)k * n + off), off, 1u,
                               t.cnt_k + (size_t)k * n + off, t.mid + (size_t)k * n, t.big + (size_t)k * n, t.ctl + 2 * k);
        }
    }
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}
int ticket_query_scan(edynhip_ctx *c, const QaTicket &t) {
    return scan_counts(c, *c->qa, 4 * t.n, t.cnt4, t.off4, t.tot, t.off4 + 4 * (size_t)t.n, nullptr);
}
int ticket_query_fill(edynhip_ctx *c, const QaTicket &t) {
    const uint32_t n = t.n;
    if (n == 0 || t.capacity == 0) return EDYNHIP_OK;
    QueryAabb &q = *c->qa;
    for (int k = 0; k < 3; ++k) {
        if (!(t.want_any & (1u << k))) continue;
        const QaArgs a = ticket_args(c, k, t.flags);
        const float4 *boxes = t.boxes_k + 2 * (size_t)k * n;
        const uint32_t *cnt = t.cnt_k + (size_t)k * n, *off = t.off_k + (size_t)k * n;
        for (uint32_t o = 0; o < n; o += kQaChunk) {
            const uint32_t m = std::min(kQaChunk, n - o);
            hipLaunchKernelGGL(k_qa_fill, dim3(nblocks(m, 256)), dim3(256), 0, c->stream, a, m, boxes + 2 * (size_t)o, cnt + o, off + o, t.ids, t.capacity);
        }
        if (a.mode == QA_TREE) {
            hipLaunchKernelGGL(k_qa_sort, dim3(std::min(n, 2048u)), dim3(64), 0, c->stream, t.mid + (size_t)k * n, t.ctl + 2 * k, cnt, off, t.ids, t.capacity, (unsigned long long *)(q.ctl + 4));
            hipLaunchKernelGGL(k_qa_scan_fill, dim3(std::min(nblocks(n, 4), 1024u)), dim3(256), 0, c->stream, a, boxes, t.big + (size_t)k * n, t.ctl + 2 * k, off, t.ids, t.capacity, (unsigned long long *)(q.ctl + 4));
        }
    }
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}
IslandView ticket_island_view(edynhip_ctx *c) {
    const QueryAabb &q = *c->qa;
    return IslandView{c->query_island && c->step_index == 0 ? c->query_island : c->b.island, q.flag, q.slot, q.imin, q.imax};
}

}  // namespace eh

using namespace eh;

static int check_query(edynhip_ctx *c, int category, uint32_t flags, const char *who) {
    if (category != EDYNHIP_QUERY_PROCEDURAL && category != EDYNHIP_QUERY_NON_PROCEDURAL && category != EDYNHIP_QUERY_ISLANDS)
        return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": unknown category").c_str());
    if (flags & ~(uint32_t)EDYNHIP_QUERY_BRUTE_FORCE) return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": unknown flag bits").c_str());
    if (c->world_shard) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, (std::string(who) + ": a shard of a multi-device world has no AABB query").c_str());
    return EDYNHIP_OK;
}

int edynhip_query_aabb_device(edynhip_ctx *c, int category, uint32_t n, const void *boxes_f4, uint32_t flags, void *offsets, void *ids,
                              uint32_t capacity, void *total) {
    if (!c || !offsets || !total || (n && !boxes_f4)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_query(c, category, flags, "edynhip_query_aabb_device"));
    EH_HIP(c, hipSetDevice(c->device));
    return run_query(c, category, n, (const float4 *)boxes_f4, flags, (uint32_t *)offsets, (uint32_t *)ids, capacity, (uint32_t *)total);
}

int edynhip_query_aabb(edynhip_ctx *c, int category, uint32_t n, const float *boxes6, uint32_t flags, uint32_t *offsets, uint32_t *ids,
                       uint32_t capacity, uint32_t *total) {
    if (!c || !offsets || !total || (n && !boxes6)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_query(c, category, flags, "edynhip_query_aabb"));
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(qa_reserve(c, n, false));
    QueryAabb &q = *c->qa;
    if (2 * (size_t)n > q.boxes_cap || (size_t)n + 1 > q.off_cap) {
        EH_HIP(c, hipStreamSynchronize(c->stream));
        q.boxes_cap = q.off_cap = 0; q.counted = false;
        EH_TRY(qalloc(c, q.d_boxes, 2 * (size_t)n)); EH_TRY(qalloc(c, q.d_off, (size_t)n + 1));
        q.boxes_cap = 2 * (size_t)n; q.off_cap = (size_t)n + 1;
    }
    if (!q.d_total) EH_TRY(qalloc(c, q.d_total, 1));
    std::vector<float4> &hb = q.stage_boxes;
    hb.resize(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes6 + 6 * (size_t)i;
        hb[2 * (size_t)i] = make_float4(b[0], b[1], b[2], 0.0f);
        hb[2 * (size_t)i + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    const bool again = q.counted && q.counted_epoch == c->state_epoch && q.counted_category == category && q.counted_flags == flags && q.counted_n == n &&
                       (n == 0 || memcmp(hb.data(), q.host_boxes.data(), 2 * (size_t)n * sizeof(float4)) == 0);
    unsigned long long tot = 0;
    if (again) {
        tot = q.counted_total;
        EH_HIP(c, hipMemcpyAsync(offsets, q.d_off, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        EH_HIP(c, hipStreamSynchronize(c->stream));
    } else {
        q.host_boxes.swap(hb);
        if (n) EH_HIP(c, hipMemcpyAsync(q.d_boxes, q.host_boxes.data(), 2 * (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        // first the counts (and the lists of the wave paths): the ids buffer on the device is sized by the total, not by the caller's capacity
        EH_TRY(run_query(c, category, n, q.d_boxes, flags, q.d_off, nullptr, 0, q.d_total, true));
        EH_HIP(c, hipMemcpyAsync(offsets, q.d_off, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        EH_HIP(c, hipMemcpyAsync(&tot, q.tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
        EH_HIP(c, hipStreamSynchronize(c->stream));
        q.counted = true; q.counted_epoch = c->state_epoch; q.counted_category = category; q.counted_flags = flags; q.counted_n = n; q.counted_total = tot;
    }
    *total = tot >= kSat ? kSat : (uint32_t)tot;
    if (!ids) return EDYNHIP_OK;
    if (tot > capacity || tot >= kSat) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_query_aabb: capacity (offsets and total are valid: size ids by *total and ask again)");
    if (tot == 0) return EDYNHIP_OK;
    if ((size_t)tot > q.ids_cap) { q.ids_cap = 0; EH_TRY(qalloc(c, q.d_ids, (size_t)tot)); q.ids_cap = (size_t)tot; }
    EH_TRY(run_query(c, category, n, q.d_boxes, flags, q.d_off, q.d_ids, (uint32_t)tot, q.d_total, false, true));
    EH_HIP(c, hipMemcpyAsync(ids, q.d_ids, (size_t)tot * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    return EDYNHIP_OK;
}

int edynhip_query_aabb_stats(edynhip_ctx *c, uint64_t *wave_sorted, uint64_t *wave_filled) {
    if (!c) return EDYNHIP_ERR_INVALID;
    unsigned long long s[2] = {0, 0};
    if (c->qa && c->qa->ctl) {
        EH_HIP(c, hipSetDevice(c->device));
        EH_HIP(c, hipMemcpyAsync(s, c->qa->ctl + 4, sizeof(s), hipMemcpyDeviceToHost, c->stream));
        EH_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (wave_sorted) *wave_sorted = s[0];
    if (wave_filled) *wave_filled = s[1];
    return EDYNHIP_OK;
}
