// Edge colouring of the contact graph and the sort of the manifolds by (colour, point count), as gfx950 kernels.
//
// NOT in the reference, which sweeps an island's rows strictly sequentially (Gauss-Seidel, island_solver.cpp:76-111). Here the contact
// graph is edge-coloured so that the manifolds of one colour share no procedural body, and every body meets its manifolds in colour
// order (solver.hip). The priorities reproduce sequential first-fit colouring in canonical pair order.
#include <algorithm>
#include "dstep.hpp"

namespace eh {
constexpr uint32_t kCsBlock = 1024, kCsKeys = 256, kCsDirectBlocks = 256, kCsSuper = 16;   // the colour sort (k_cs_*)
// Edge priority for the colouring rounds: lower edge index wins, which reproduces sequential first-fit
// colouring in canonical pair order (near-optimal colour counts on stacked scenes: max degree or +1) at the
// price of more rounds when a whole scene is coloured from scratch; steady state only colours new edges.
DI uint64_t edge_prio(uint32_t e) { return (uint64_t)(0xFFFFFFFFu - e); }

// ------------------------------------------------------------------ colouring
// In every island that has an edge to colour in this step (a new or re-activated contact) the top colour carried over from the last
// step is released and first-fit again, so colour classes freed by vanished contacts are reclaimed when the island next changes and
// the colour count (= dependent hops per sweep) does not drift upwards - while an island in which nothing happened keeps its
// colouring untouched (4096 settled mini-piles: nothing to recolour). Per ISLAND, not per world: an island is coloured - and
// therefore solved - the same way whatever else the world holds, so a shard of the world (edyn_amd/parallel.py) steps exactly like
// the whole. k_col_tops finds each island's top colour (+ 1; .x) and whether it has an uncoloured active edge (.y), k_col_prepare releases.
__device__ __forceinline__ uint32_t manifold_label(uint32_t a, uint32_t b, uint32_t fa, const uint32_t *__restrict__ island) { return island[is_dynamic(fa) ? a : b]; }
__global__ void __launch_bounds__(1024) k_col_tops(uint32_t M, const uint32_t *__restrict__ info, const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                                                   const uint32_t *__restrict__ flags, const uint32_t *__restrict__ island, uint2 *isl_top, uint32_t *cs_sup) {
    __shared__ uint32_t s_label[16], s_top[16];
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    // (first kernel of the colouring chain: also clears the colour sort's super-block key counts, k_cs_hist<true>)
    for (uint32_t g = m; g < (kCsDirectBlocks / kCsSuper) * kCsKeys; g += gridDim.x * blockDim.x) cs_sup[g] = 0u;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t label = 0xFFFFFFFFu, top = 0;
    if (m < M) {
        const uint32_t in = info[m], np = in & 0xFF, col = in >> 8;
        const uint32_t a = bA[m], b = bB[m], fa = flags[a], fb = flags[b];
        if (np > 0 && !edge_asleep(fa, fb)) {
            const uint32_t l = manifold_label(a, b, fa, island);
            if (col != kNoColour) { label = l; top = col + 1; }
            else isl_top[l].y = 1u;   // the island has something to colour in this step (identical plain stores)
        }
    }
    // Neighbours in the canonical order mostly share their island. A wave of one island hands its maximum to the workgroup, which
    // issues one atomic per run of equal labels (a big island: one per 1024 manifolds instead of thousands on one address); a wave
    // that spans islands issues one atomic per island it touches. A plain look comes first: once an island's top colour has landed
    // the others have nothing to add.
    auto post = [&](uint32_t l, uint32_t t) { if (__atomic_load_n(&isl_top[l].x, __ATOMIC_RELAXED) < t) atomicMax(&isl_top[l].x, t); };
    uint64_t todo = __ballot(top != 0);
    uint32_t w_label = 0xFFFFFFFFu, w_top = 0;
    if (todo) {
        const uint32_t l0 = __shfl(label, __ffsll((long long)todo) - 1);
        if (__ballot(top != 0 && label == l0) == todo) {   // one island
            uint32_t t = top;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t = max(t, (uint32_t)__shfl_xor(t, off));
            w_label = l0; w_top = t;
        } else {
            while (todo) {
                const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1, l = __shfl(label, leader);
                const bool mine = top != 0 && label == l;
                uint32_t t = mine ? top : 0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t = max(t, (uint32_t)__shfl_xor(t, off));
                if (lane == leader) post(l, t);
                todo &= ~__ballot(mine);
            }
        }
    }
    if (lane == 0) { s_label[wave] = w_label; s_top[wave] = w_top; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t l = 0xFFFFFFFFu, t = 0;
        for (int w = 0; w < 16; ++w) {
            if (s_top[w] == 0) continue;
            if (s_label[w] != l) { if (t) post(l, t); l = s_label[w]; t = 0; }
            t = max(t, s_top[w]);
        }
        if (t) post(l, t);
    }
}
__global__ void __launch_bounds__(1024) k_col_prepare(uint32_t M, uint32_t *__restrict__ info, const uint32_t *__restrict__ bA,
                              const uint32_t *__restrict__ bB, const uint32_t *__restrict__ flags, uint64_t *used,
                              uint64_t *best0, uint64_t *best1, Counters *cnt, const uint32_t *__restrict__ island, const uint2 *__restrict__ isl_top,
                              uint32_t *unc_list) {
    uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t unc = 0;
    if (m < M) {
        uint32_t in = info[m];
        uint32_t np = in & 0xFF, col = in >> 8;
        const uint32_t a = bA[m], b = bB[m];
        const uint32_t fa = flags[a], fb = flags[b];
        // a sleeping manifold is out of the solve but keeps (and blocks) its colour for when its island wakes
        const bool asleep = edge_asleep(fa, fb);
        if (np > 0 && col != kNoColour && !asleep) {
            const uint2 top = isl_top[manifold_label(a, b, fa, island)];
            if (top.y && top.x >= 2 && col + 1 == top.x) { col = kNoColour; info[m] = np | (kNoColour << 8); }
        }
        if (np > 0) {
            bool da = is_dynamic(fa), db = is_dynamic(fb);
            if (col != kNoColour) {
                if (da) atomicOr((unsigned long long *)&used[a], 1ull << col);
                if (db) atomicOr((unsigned long long *)&used[b], 1ull << col);
            } else if (!asleep) {
                unc = 1;
                if (da) { best0[a] = 0; best1[a] = 0; }
                if (db) { best0[b] = 0; best1[b] = 0; }
            }
        }
    }
    // list the uncoloured edges for k_col_rounds (beyond its capacity only the count matters): one pair of atomics per WORKGROUP - a
    // restless scene has an uncoloured edge in almost every wave, and thousands of atomics on one cache line cost more than the kernel
    __shared__ uint32_t wcount[16], wbase;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t mask = __ballot(unc != 0);
    if (lane == 0) wcount[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) total += wcount[w];
        wbase = total ? atomicAdd(&cnt->unc_count, total) : 0u;
        if (total) atomicAdd(&cnt->uncoloured, total);
    }
    __syncthreads();
    if (unc) {
        uint32_t at = wbase + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) at += wcount[w];
        if (at < kColUncCap) unc_list[at] = m;
    }
}
// The rounds for a list of uncoloured edges that one workgroup can hold - the steady state: some hundred (a restless heap: some
// thousand) new contacts per step - run in one workgroup with workgroup barriers between the phases instead of two launches per
// round; same rule, same result as k_col_best / k_col_assign. The edges' endpoints sit in LDS (index | dynamic << 31), the list is
// compacted as edges take their colour (a round only visits what is still uncoloured). The endpoint marks carry the round in their upper
// half - (round + 1) << 32 | priority - so a mark of an earlier round loses against any mark of this one and nothing has to be zeroed
// between rounds (round 5: the workgroup is bound by the memory requests one CU can issue - a restless heap of polyhedra lists 15 000
// edges per step and still has two thirds of them after three rounds; the zeroing stores were two of six requests per edge and round).
// Longer lists, and what is left after max_rounds, go to the multi-block rounds (the host sees cnt->uncoloured != 0).
__global__ void __launch_bounds__(1024) k_col_rounds(uint32_t *info, const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                                                     const uint32_t *__restrict__ flags, uint64_t *best0, uint64_t *best1, uint64_t *used, Counters *cnt,
                                                     uint32_t *list, uint32_t cap, uint32_t max_rounds) {
    extern __shared__ uint32_t col_lds[];   // ea[cap], eb[cap]
    uint32_t *ea = col_lds, *eb = col_lds + cap;
    __shared__ uint32_t live, wr;
    const uint32_t n0 = cnt->unc_count;
    if (n0 == 0 || n0 > cap) { if (threadIdx.x == 0) cnt->col_wg_rounds = 0; return; }
    for (uint32_t e = threadIdx.x; e < n0; e += blockDim.x) {
        const uint32_t m = list[e], a = bA[m], b = bB[m];
        ea[e] = a | (is_dynamic(flags[a]) ? 0x80000000u : 0u);
        eb[e] = b | (is_dynamic(flags[b]) ? 0x80000000u : 0u);
    }
    if (threadIdx.x == 0) live = n0;
    __syncthreads();
    auto ld = [](const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };   // other waves' stores: not through a stale L1 line
    auto ld32 = [](const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    uint32_t round = 0;
    for (; round < max_rounds; ++round) {
        const uint32_t n = live;
        if (n == 0) break;
        uint64_t *cur = best0;
        const uint64_t stamp = (uint64_t)(round + 1u) << 32;   // (edge_prio fits the lower half)
        for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) {           // phase 1: every endpoint learns its best uncoloured edge
            const uint64_t pr = stamp | edge_prio(list[e]);
            const uint32_t a = ea[e], b = eb[e];
            if (a >> 31) atomicMax((unsigned long long *)&cur[a & 0x7FFFFFFFu], pr);
            if (b >> 31) atomicMax((unsigned long long *)&cur[b & 0x7FFFFFFFu], pr);
        }
        if (threadIdx.x == 0) wr = 0;
        __threadfence_block(); __syncthreads();   // one workgroup, one CU: its stores only have to reach L2 before the other waves' (atomic) loads
        for (uint32_t base = 0; base < n; base += blockDim.x) {           // phase 2: edges that are best at both ends take a colour, the others stay listed
            const uint32_t e = base + threadIdx.x;
            bool keep = false;
            uint32_t m = 0, a = 0, b = 0;
            if (e < n) {
                m = list[e]; a = ea[e]; b = eb[e];
                const bool da = a >> 31, db = b >> 31;
                const uint32_t ia = a & 0x7FFFFFFFu, ib = b & 0x7FFFFFFFu;
                const uint64_t pr = stamp | edge_prio(m);
                if ((da && ld(&cur[ia]) != pr) || (db && ld(&cur[ib]) != pr)) keep = true;
                else {
                    const uint64_t busy = (da ? ld(&used[ia]) : 0ull) | (db ? ld(&used[ib]) : 0ull);
                    const uint64_t avail = ~busy & ((1ull << kSerialColour) - 1ull);
                    const uint32_t c = avail ? (uint32_t)__ffsll((long long)avail) - 1 : kSerialColour;   // nothing free: the serial bucket
                    info[m] = (ld32(&info[m]) & 0xFF) | (c << 8);
                    if (da) atomicOr((unsigned long long *)&used[ia], 1ull << c);
                    if (db) atomicOr((unsigned long long *)&used[ib], 1ull << c);
                }
            }
            __syncthreads();   // this block of the list has been read: its survivors may now be written over the front of it
            const uint64_t mask = __ballot(keep);
            if (mask) {
                const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)mask) - 1;
                uint32_t at = 0;
                if (lane == leader) at = atomicAdd(&wr, (uint32_t)__popcll(mask));
                at = __shfl(at, leader) + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (keep) { list[at] = m; ea[at] = a; eb[at] = b; }
            }
        }
        __threadfence_block(); __syncthreads();
        if (threadIdx.x == 0) live = wr;
        __syncthreads();
    }
    const uint32_t left = live;
    if (left) {   // handed to the multi-block rounds, which start from clean marks in both arrays
        for (uint32_t e = threadIdx.x; e < left; e += blockDim.x) {
            const uint32_t a = ea[e], b = eb[e];
            if (a >> 31) { best0[a & 0x7FFFFFFFu] = 0; best1[a & 0x7FFFFFFFu] = 0; }
            if (b >> 31) { best0[b & 0x7FFFFFFFu] = 0; best1[b & 0x7FFFFFFFu] = 0; }
        }
    }
    if (threadIdx.x == 0) { cnt->uncoloured = left; cnt->col_wg_rounds = round; }
}
// Round 6, an experiment kept behind EDYNHIP_COL_LDS=1 (measured: 3 % faster on the polyhedron heap, 1-2 us SLOWER per step on every pile - the
// 159 KB of LDS it asks for and its clearing - so k_col_rounds above stays the default; the two are compared by
// test_colouring_rounds_in_lds_and_in_global_memory_colour_alike): the same rounds with the endpoint marks in LDS. The kernel above spends its time on the memory requests one CU can issue - eight
// scattered 8-byte requests per listed edge and round (two marks set, two read, the list read twice and rewritten), 15 000 edges and ~32
// rounds on a restless heap. Here the list, the edges' endpoints and the marks live in LDS; global memory is touched once per edge, when it
// takes its colour. The marks are a HASHED table (slot = hash(body), 4 bytes: the priority): two bodies may share a slot, and then an edge is
// "best" only if it beats the uncoloured edges of every body in its two slots - a stricter test than the rule's, so an edge may take its
// colour a round later, never earlier: it still takes it after all its higher-priority neighbours and before all lower ones, and the result
// is the greedy colouring in priority order whatever the rounds were (winners of one round are never adjacent). Every thread owns the edges
// t, t + 1024, ... and keeps its survivors packed at the front of that column: no list compaction across threads, three barriers per round.
__global__ void __launch_bounds__(1024) k_col_rounds_lds(uint32_t *info, const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                                                     const uint32_t *__restrict__ flags, uint64_t *used, Counters *cnt,
                                                     const uint32_t *__restrict__ list, uint32_t cap, uint32_t lds_words, uint32_t max_rounds) {
    extern __shared__ uint32_t col_lds[];   // em[n0] manifold, es[n0] endpoint slots (slot A | dynamic A << 15 | slot B << 16 | dynamic B << 31), mark[T]
    __shared__ uint32_t alive[2], left_sum;
    const uint32_t n0 = cnt->unc_count;
    if (n0 == 0 || n0 > cap) { if (threadIdx.x == 0) cnt->col_wg_rounds = 0; return; }
    uint32_t *em = col_lds, *es = col_lds + n0, *mark = col_lds + 2 * n0;
    uint32_t T = 1024, bits = 10;   // table size: what the workgroup's LDS leaves, at most 2^15 slots, no more than ~16 per edge (it is cleared once)
    while (T < 32768u && 2 * T <= lds_words - 2 * n0 && T < 16u * n0) { T *= 2; ++bits; }
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < T; i += blockDim.x) mark[i] = 0;
    uint32_t mine = 0;   // live edges of this thread: em[tid + k * 1024], k < mine (its share of the list, packed at the front of its column)
    for (uint32_t e = tid; e < n0; e += blockDim.x) {
        const uint32_t m = list[e], a = bA[m], b = bB[m];
        const uint32_t sa = (a * 0x9E3779B1u) >> (32u - bits), sb = (b * 0x9E3779B1u) >> (32u - bits);
        const uint32_t to = tid + mine++ * blockDim.x;
        em[to] = m;
        es[to] = sa | (is_dynamic(flags[a]) ? 0x8000u : 0u) | (sb << 16) | (is_dynamic(flags[b]) ? 0x80000000u : 0u);
    }
    if (tid < 2) alive[tid] = 0;
    if (tid == 0) left_sum = 0;
    __syncthreads();
    auto ld = [](const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };   // other waves' atomics: not through a stale L1 line
    auto ld32 = [](const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    uint32_t round = 0;
    for (; round < max_rounds; ++round) {
        for (uint32_t k = 0; k < mine; ++k) {                                // phase 1: every slot learns the best uncoloured edge of its bodies
            const uint32_t e = tid + k * blockDim.x, s = es[e], pr = (uint32_t)edge_prio(em[e]);
            if (s & 0x8000u) atomicMax(&mark[s & 0x7FFFu], pr);
            if (s >> 31) atomicMax(&mark[(s >> 16) & 0x7FFFu], pr);
        }
        __syncthreads();
        if (tid == 0) alive[(round + 1) & 1] = 0;
        // phase 2: an edge that is best in both its slots takes its colour. The winners of a thread are taken four at a time with their loads
        // issued together - bodies and point count, then the bodies' colour masks: two dependent round trips per batch, where one winner after
        // the other paid them per edge (a thread owns up to 16 listed edges; winners of a round are never adjacent, so their masks are independent)
        for (uint32_t k = 0;;) {
            uint32_t nw = 0, we[4];
            for (; k < mine && nw < 4u; ++k) {
                const uint32_t e = tid + k * blockDim.x, s = es[e], pr = (uint32_t)edge_prio(em[e]);
                if (((s & 0x8000u) && mark[s & 0x7FFFu] != pr) || ((s >> 31) && mark[(s >> 16) & 0x7FFFu] != pr)) continue;
                we[nw++] = e;
            }
            if (nw == 0) break;
            uint32_t wm[4], ws[4], ia[4], ib[4], in[4];
            uint64_t busy[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (j < nw) { wm[j] = em[we[j]]; ws[j] = es[we[j]]; ia[j] = bA[wm[j]]; ib[j] = bB[wm[j]]; in[j] = ld32(&info[wm[j]]); }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (j < nw) busy[j] = ((ws[j] & 0x8000u) ? ld(&used[ia[j]]) : 0ull) | ((ws[j] >> 31) ? ld(&used[ib[j]]) : 0ull);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (j < nw) {
                    const uint64_t avail = ~busy[j] & ((1ull << kSerialColour) - 1ull);
                    const uint32_t c = avail ? (uint32_t)__ffsll((long long)avail) - 1 : kSerialColour;   // nothing free: the serial bucket
                    info[wm[j]] = (in[j] & 0xFF) | (c << 8);
                    // its marks go at once (nobody else can equal them: the others in these slots read either this priority or zero and stay)
                    if (ws[j] & 0x8000u) { atomicOr((unsigned long long *)&used[ia[j]], 1ull << c); mark[ws[j] & 0x7FFFu] = 0; }
                    if (ws[j] >> 31) { atomicOr((unsigned long long *)&used[ib[j]], 1ull << c); mark[(ws[j] >> 16) & 0x7FFFu] = 0; }
                    em[we[j]] = 0xFFFFFFFFu;
                }
        }
        __threadfence_block(); __syncthreads();   // the marks have been read; the colours' atomics are at the L2 before the next round reads `used`
        uint32_t kept = 0;
        for (uint32_t k = 0; k < mine; ++k) {                                // the survivors clear their slots and move to the front of the column
            const uint32_t e = tid + k * blockDim.x, m = em[e];
            if (m == 0xFFFFFFFFu) continue;
            const uint32_t s = es[e];
            if (s & 0x8000u) mark[s & 0x7FFFu] = 0;
            if (s >> 31) mark[(s >> 16) & 0x7FFFu] = 0;
            const uint32_t to = tid + kept * blockDim.x;
            if (to != e) { em[to] = m; es[to] = s; }
            ++kept;
        }
        mine = kept;
        if (__ballot(mine != 0) && (tid & 63u) == 0) alive[round & 1] = 1;
        __syncthreads();
        if (!alive[round & 1]) { ++round; break; }
    }
    // what max_rounds left over goes to the multi-block rounds (their marks were cleared by k_col_prepare and never touched here)
    uint32_t left = mine;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) left += __shfl_xor(left, off);
    if ((tid & 63u) == 0 && left) atomicAdd(&left_sum, left);
    __syncthreads();
    if (tid == 0) { cnt->uncoloured = left_sum; cnt->col_wg_rounds = round; }
}
__global__ void k_col_best(uint32_t M, const uint32_t *__restrict__ info, const uint32_t *__restrict__ bA,
                           const uint32_t *__restrict__ bB, const uint32_t *__restrict__ flags, uint64_t *best_cur,
                           uint64_t *best_next, const Counters *cnt) {
    if (cnt->uncoloured == 0) return;
    uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    uint32_t in = info[m];
    if ((in & 0xFF) == 0 || (in >> 8) != kNoColour) return;
    uint32_t a = bA[m], b = bB[m];
    if (edge_asleep(flags[a], flags[b])) return;
    uint64_t pr = edge_prio(m);
    if (is_dynamic(flags[a])) { atomicMax((unsigned long long *)&best_cur[a], pr); best_next[a] = 0; }
    if (is_dynamic(flags[b])) { atomicMax((unsigned long long *)&best_cur[b], pr); best_next[b] = 0; }
}
__global__ void k_col_assign(uint32_t M, uint32_t *info, const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                             const uint32_t *__restrict__ flags, const uint64_t *__restrict__ best_cur, uint64_t *used,
                             Counters *cnt) {
    if (cnt->uncoloured == 0) return;
    uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t done = 0;
    if (m < M) {
        uint32_t in = info[m];
        if ((in & 0xFF) != 0 && (in >> 8) == kNoColour) {
            uint32_t a = bA[m], b = bB[m];
            bool da = is_dynamic(flags[a]), db = is_dynamic(flags[b]);
            uint64_t pr = edge_prio(m);
            if (!edge_asleep(flags[a], flags[b]) && !(da && best_cur[a] != pr) && !(db && best_cur[b] != pr)) {
                uint64_t busy = (da ? used[a] : 0ull) | (db ? used[b] : 0ull);
                const uint64_t avail = ~busy & ((1ull << kSerialColour) - 1ull);
                const uint32_t c = avail ? (uint32_t)__ffsll((long long)avail) - 1 : kSerialColour;   // nothing free: the serial bucket
                info[m] = (in & 0xFF) | (c << 8);
                if (da) used[a] |= 1ull << c;
                if (db) used[b] |= 1ull << c;
                done = 1;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) done += __shfl_xor(done, off);
    if ((threadIdx.x & 63) == 0 && done) atomicSub(&cnt->uncoloured, done);
}
DI uint32_t colour_key(uint32_t m, const uint32_t *__restrict__ info, const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                       const uint32_t *__restrict__ flags, bool sleeping) {
    // within a colour, manifolds are grouped by point count (4 first): the solve kernels then know a lane's point
    // count from its position alone (no dependent load) and waves are uniform in it
    uint32_t in = info[m];
    uint32_t np = in & 0xFF;
    if (sleeping && np && edge_asleep(flags[bA[m]], flags[bB[m]])) np = 0;   // not part of this step's solve
    return np ? (((in >> 8) << 2) | (4u - np)) : 0xFFu;
}
// Stable counting sort of the manifolds by (colour, point count) key - at most 256 distinct keys. (rocPRIM's radix sort
// falls back to a merge sort for an 8-bit key range: 1 block-sort + 16 merge launches, ~90 us per step.)
//  k_cs_hist:    per 1024-element block, the count of every key          -> hist[key * nblocks + block]
//  scan_u32:     exclusive scan of that key-major table                   -> where each (key, block) run starts
//  k_cs_scatter: every element's slot = its run's start + its rank among the block's earlier elements with its key
//  Scenes of up to kCsDirectBlocks blocks (the headline pile: 174) take two launches instead of five (round 5): the
//  histogram table is block-major there and k_cs_hist<true> also accumulates the key counts of every kCsSuper blocks (`sup`, integer
//  sums: the same values whatever the order); k_cs_scatter<true> gets the run starts of its block from at most 16 + 15 table rows,
//  builds the key starts from the totals, and block 0 publishes the colour ranges (k_col_offsets' work). No library scan on the hot path.
template <bool DIRECT>
__global__ void __launch_bounds__(kCsBlock) k_cs_hist(uint32_t M, uint32_t *keys, uint32_t *hist, uint32_t nblocks, const uint32_t *__restrict__ info,
                                                      const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                                                      const uint32_t *__restrict__ flags, bool sleeping, uint32_t *sup) {
    __shared__ uint32_t h[kCsKeys];
    if (threadIdx.x < kCsKeys) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t m = blockIdx.x * kCsBlock + threadIdx.x;
    if (m < M) {
        const uint32_t key = colour_key(m, info, bA, bB, flags, sleeping);
        keys[m] = key;
        atomicAdd(&h[key & 0xFFu], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kCsKeys) {
        hist[DIRECT ? blockIdx.x * kCsKeys + threadIdx.x : threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
        if (DIRECT && h[threadIdx.x]) atomicAdd(&sup[(blockIdx.x / kCsSuper) * kCsKeys + threadIdx.x], h[threadIdx.x]);
    }
}
template <bool DIRECT>
__global__ void __launch_bounds__(kCsBlock) k_cs_scatter(uint32_t M, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ start,
                                                         uint32_t nblocks, uint32_t *keys_sorted, uint32_t *order, Counters *cnt, const uint32_t *__restrict__ sup) {
    __shared__ uint32_t base[kCsKeys];
    if (DIRECT) {   // `start` is the block-major histogram table
        __shared__ uint32_t wsum[4], part[kCsKeys];
        uint32_t before = 0, total = 0;
        {   // lanes 0..255: the super-block rows (key totals; what lies before this block's super-block); lanes 256..511: the rows of
            // the blocks before this one inside its super-block - at most 16 + 15 independent loads per key
            const uint32_t k = threadIdx.x & (kCsKeys - 1), q = threadIdx.x >> 8, sb = blockIdx.x / kCsSuper, nsup = (nblocks + kCsSuper - 1) / kCsSuper;
            if (q == 0) {
                uint32_t v[kCsDirectBlocks / kCsSuper];
#pragma unroll
                for (uint32_t u = 0; u < kCsDirectBlocks / kCsSuper; ++u) v[u] = u < nsup ? sup[u * kCsKeys + k] : 0u;
#pragma unroll
                for (uint32_t u = 0; u < kCsDirectBlocks / kCsSuper; ++u) { total += v[u]; before += u < sb ? v[u] : 0u; }
            } else if (q == 1) {
                uint32_t v[kCsSuper], inner = 0;
#pragma unroll
                for (uint32_t u = 0; u < kCsSuper; ++u) { const uint32_t b = sb * kCsSuper + u; v[u] = b < blockIdx.x ? start[b * kCsKeys + k] : 0u; }
#pragma unroll
                for (uint32_t u = 0; u < kCsSuper; ++u) inner += v[u];
                part[k] = inner;
            }
        }
        __syncthreads();
        if (threadIdx.x < kCsKeys) before += part[threadIdx.x];
        // exclusive scan of the 256 key totals (lanes 0..255 = waves 0..3)
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint32_t inc = total;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(inc, d); if ((int)lane >= d) inc += u; }
        if (wave < 4 && lane == 63) wsum[wave] = inc;
        __syncthreads();
        if (threadIdx.x < kCsKeys) {
            uint32_t key_start = inc - total;
            for (uint32_t w = 0; w < wave; ++w) key_start += wsum[w];
            base[threadIdx.x] = key_start + before;
            if (blockIdx.x == 0 && threadIdx.x < 4 * kMaxContactColours && total) {   // what k_col_offsets reads off the sorted keys
                cnt->colour_start[threadIdx.x] = key_start; cnt->colour_end[threadIdx.x] = key_start + total;
            }
        }
    } else if (threadIdx.x < kCsKeys) base[threadIdx.x] = start[threadIdx.x * nblocks + blockIdx.x];
    __syncthreads();
    const uint32_t m = blockIdx.x * kCsBlock + threadIdx.x;
    const bool valid = m < M;
    const uint32_t key = valid ? (keys[m] & 0xFFu) : 0xFFFFFFFFu;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // rank among the lower lanes of this wave with the same key, and the wave's count of that key (at its first lane)
    uint32_t rank = 0, count = 0;
    bool first = false;
    uint64_t todo = __ballot(valid);
    while (todo) {
        const uint32_t k = __shfl(key, __ffsll((long long)todo) - 1);
        const uint64_t same = __ballot(valid && key == k);
        if (valid && key == k) {
            rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            count = (uint32_t)__popcll(same);
            first = rank == 0;
        }
        todo &= ~same;
    }
    for (uint32_t w = 0; w < kCsBlock / 64; ++w) {   // waves take their turns in order: keeps the sort stable
        if (wave == w && valid) {
            const uint32_t pos = base[key] + rank;
            keys_sorted[pos] = key; order[pos] = m;
        }
        __syncthreads();
        if (wave == w && valid && first) base[key] += count;
        __syncthreads();
    }
}
__global__ void k_col_offsets(uint32_t M, const uint32_t *__restrict__ keys_sorted, Counters *cnt) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M) return;
    uint32_t c = keys_sorted[p];
    if (c >= 4 * kMaxContactColours) return;
    if (p == 0 || keys_sorted[p - 1] != c) cnt->colour_start[c] = p;
    if (p == M - 1 || keys_sorted[p + 1] != c) cnt->colour_end[c] = p + 1;
}

// `between`: called once, after the steady-state colouring and its counter publish are enqueued and before the host waits for the
// counters - what it enqueues runs while the answer travels (it must not depend on the answer). *first_final tells the caller whether
// the counters of that first publish were the final ones (no multi-block colouring rounds, no second sort).
int colour_contacts(edynhip_ctx *c, const std::function<void()> &between, bool *first_final) {
    *first_final = false;
    hipStream_t s = c->stream;
    const uint32_t M = c->num_manifolds, n = c->b.n;
    Manifolds &mf = c->m[c->cur];
    c->num_active = 0;
    if (M == 0) { c->num_colours = 0; return EDYNHIP_OK; }
    if (!c->full_step) {   // inside edynhip_step: `used` was cleared by the previous k_finish, the counters by k_step_reset
        EH_HIP(c, hipMemsetAsync(c->used, 0, (size_t)n * sizeof(uint64_t), s));
        EH_HIP(c, hipMemsetAsync(c->isl_top, 0, (size_t)n * sizeof(uint2), s));
        EH_HIP(c, hipMemsetAsync(&c->cnt->uncoloured, 0, 2 * sizeof(uint32_t), s));   // uncoloured, colour_overflow
        EH_HIP(c, hipMemsetAsync(c->cnt->colour_start, 0, 8 * kMaxColours * sizeof(uint32_t), s));
    }
    hipLaunchKernelGGL(k_col_tops, dim3(blocks(M, 1024)), dim3(1024), 0, s, M, mf.info, mf.bodyA, mf.bodyB, c->b.flags, c->b.island, c->isl_top, c->cs_sup);
    hipLaunchKernelGGL(k_col_prepare, dim3(blocks(M, 1024)), dim3(1024), 0, s, M, mf.info, mf.bodyA, mf.bodyB, c->b.flags, c->used, c->best[0], c->best[1], c->cnt, c->b.island, c->isl_top, c->col_unc);
    uint32_t round = 0, total_rounds = 0;
    auto run_rounds = [&](uint32_t count) {
        for (uint32_t r = 0; r < count; ++r, ++round) {
            uint64_t *bc = c->best[round & 1], *bn = c->best[(round + 1) & 1];
            hipLaunchKernelGGL(k_col_best, dim3(blocks(M, 256)), dim3(256), 0, s, M, mf.info, mf.bodyA, mf.bodyB, c->b.flags, bc, bn, c->cnt);
            hipLaunchKernelGGL(k_col_assign, dim3(blocks(M, 256)), dim3(256), 0, s, M, mf.info, mf.bodyA, mf.bodyB, c->b.flags, bc, c->used, c->cnt);
        }
        total_rounds += count;
    };
    bool first = true;
    auto sort_and_fetch = [&]() -> int {
        {
            const uint32_t nb = blocks(M, kCsBlock);
            const bool direct_env = c->knobs.direct_sort;   // developer knob (A/B)
            if (nb <= kCsDirectBlocks && direct_env) {
                c->paths |= EDYNHIP_PATH_SORT_DIRECT;
                if (!first) EH_HIP(c, hipMemsetAsync(c->cs_sup, 0, (size_t)(kCsDirectBlocks / kCsSuper) * kCsKeys * sizeof(uint32_t), s));   // (the step's first sort: cleared by k_col_tops)
                hipLaunchKernelGGL(k_cs_hist<true>, dim3(nb), dim3(kCsBlock), 0, s, M, c->col_keys, c->cs_hist, nb, mf.info, mf.bodyA, mf.bodyB, c->b.flags, c->sleeping, c->cs_sup);
                hipLaunchKernelGGL(k_cs_scatter<true>, dim3(nb), dim3(kCsBlock), 0, s, M, c->col_keys, c->cs_hist, nb, c->col_keys_sorted, c->rows.order, c->cnt, c->cs_sup);
            } else {
                c->paths |= EDYNHIP_PATH_SORT_LIBRARY;
                hipLaunchKernelGGL(k_cs_hist<false>, dim3(nb), dim3(kCsBlock), 0, s, M, c->col_keys, c->cs_hist, nb, mf.info, mf.bodyA, mf.bodyB, c->b.flags, c->sleeping, (uint32_t *)nullptr);
                EH_TRY(scan_u32(c, c->cs_hist, c->cs_start, kCsKeys * nb));
                hipLaunchKernelGGL(k_cs_scatter<false>, dim3(nb), dim3(kCsBlock), 0, s, M, c->col_keys, c->cs_start, nb, c->col_keys_sorted, c->rows.order, c->cnt, (const uint32_t *)nullptr);
                hipLaunchKernelGGL(k_col_offsets, dim3(blocks(M, 256)), dim3(256), 0, s, M, c->col_keys_sorted, c->cnt);
            }
        }
        uint32_t ticket = 0;
        EH_TRY(publish_counters(c, sizeof(Counters), &ticket));
        if (first) between();
        first = false;
        EH_TRY(wait_counters(c, ticket));
        return EDYNHIP_OK;
    };
    // Steady state: the few new edges are coloured by one workgroup (k_col_rounds) and ONE fetch brings the offsets; what it
    // could not finish (a long list, or more rounds than it runs) is left to the multi-block rounds below.
    const bool col_lds_env = c->knobs.col_lds;   // developer knob (A/B): the rounds with their marks in a hashed LDS table (k_col_rounds)
    constexpr uint32_t kColMinTable = 8192;   // mark slots the longest list still leaves room for
    if (c->col_lds_edges == 0) {   // the listed edges and the mark table live in LDS: as much as one workgroup may have (8 bytes per edge + 4 per slot)
        int max_lds = 0;
        (void)hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device);
        uint32_t bytes = max_lds > 65536 ? (uint32_t)max_lds - 1024u : 48u * 1024u;
        const void *fn = col_lds_env ? (const void *)k_col_rounds_lds : (const void *)k_col_rounds;
        if (bytes > 48u * 1024u && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            (void)hipGetLastError();
            bytes = 48u * 1024u;
        }
        c->col_lds_bytes = bytes;
        c->col_lds_edges = std::min<uint32_t>(kColUncCap, (bytes - (col_lds_env ? 4u * kColMinTable : 0u)) / 8u);
    }
    if (col_lds_env)
        hipLaunchKernelGGL(k_col_rounds_lds, dim3(1), dim3(1024), (size_t)c->col_lds_bytes, s, mf.info, mf.bodyA, mf.bodyB, c->b.flags, c->used, c->cnt,
                           c->col_unc, c->col_lds_edges, c->col_lds_bytes / 4u, 256u);
    else
        hipLaunchKernelGGL(k_col_rounds, dim3(1), dim3(1024), (size_t)c->col_lds_edges * 8u, s, mf.info, mf.bodyA, mf.bodyB, c->b.flags, c->best[0], c->best[1], c->used, c->cnt,
                           c->col_unc, c->col_lds_edges, 256u);
    EH_TRY(sort_and_fetch());
    *first_final = c->cnt_host->uncoloured == 0;
    if (c->cnt_host->uncoloured != 0) {
        uint32_t batch = 4;
        while (c->cnt_host->uncoloured != 0) {
            if (c->cnt_host->colour_overflow) break;
            run_rounds(batch);
            if (batch < 64) batch *= 2;   // a scene coloured from scratch needs hundreds of rounds; steady state needs none
            EH_TRY(fetch_counters(c, 8 * sizeof(uint32_t)));
            if (total_rounds > 65536) return set_error(c, EDYNHIP_ERR_COLOURS, "colouring did not converge");
        }
        EH_HIP(c, hipMemsetAsync(c->cnt->colour_start, 0, 8 * kMaxColours * sizeof(uint32_t), s));
        EH_TRY(sort_and_fetch());
    }
    // (no contact count is an error any more: what does not fit the 62 parallel colours goes to the serial bucket, ctx.hpp)
    c->stats.colour_rounds = total_rounds + c->cnt_host->col_wg_rounds;
    uint32_t nc = 0, na = 0;
    for (uint32_t k = 0; k < kMaxColours; ++k) {
        uint32_t begin = 0xFFFFFFFFu, pos = 0, cnt4[4];
        for (uint32_t g = 0; g < 4; ++g) {
            const uint32_t a = c->cnt_host->colour_start[4 * k + g], e = c->cnt_host->colour_end[4 * k + g];
            cnt4[g] = e - a;
            if (e > a && a < begin) begin = a;
        }
        if (begin == 0xFFFFFFFFu) { c->colour_start[k] = c->colour_end[k] = 0; continue; }
        c->colour_start[k] = begin;
        pos = begin;
        for (uint32_t g = 0; g < 3; ++g) { pos += cnt4[g]; c->colour_split[k][g] = pos; }
        c->colour_end[k] = pos + cnt4[3];
        nc = k + 1;
        na = c->colour_end[k] > na ? c->colour_end[k] : na;
    }
    c->num_colours = nc;
    c->num_active = na;
    return EDYNHIP_OK;
}

}  // namespace eh
