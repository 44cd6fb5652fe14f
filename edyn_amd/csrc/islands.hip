// Island labelling (connected components of the constraint graph) and island sleeping, as gfx950 kernels.
//
// Reference functions reproduced (arithmetic order kept):
//   island labelling            src/edyn/simulation/island_manager.cpp:117-350 (connected components; static nodes do not connect)
//   sleeping                    src/edyn/simulation/island_manager.cpp:524-623 (k_sleep_*)
//
// What is NOT in the reference: the labels come from a lock-free union-find over the bodies and are kept up to date incrementally
// (CC_* below); the reference maintains its islands with graph traversals on the host.
#include "dstep.hpp"

namespace eh {

// ------------------------------------------------------------------ islands (lock-free union-find)
// Links always point to a SMALLER body index and only ever move towards the root, so any value ever stored in
// parent[x] is an ancestor of x (or x itself) for the rest of the launch. Plain, possibly stale (per-CU L1 / per-XCD
// L2) loads are therefore safe for the walks: a stale value is merely a longer path. Only the hook itself must be
// exact - it is a device-scope compare-and-swap on the true memory value, and on failure the walk continues from the
// fresh value it returned. (Agent-scope atomic loads here were measured ~8x slower: every step went to the fabric.)
DI uint32_t cc_find(uint32_t *parent, uint32_t x) {
    uint32_t p = parent[x];
    while (p != x) {
        const uint32_t gp = parent[p];
        if (gp != p) parent[x] = gp;   // path halving; racing writers all store ancestors
        x = p; p = gp;
    }
    return x;
}
DI bool cc_union(uint32_t *parent, uint32_t a, uint32_t b) {   // true: this call joined two trees (the edge certifies the union)
    uint32_t ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        if (ra < rb) { const uint32_t t = ra; ra = rb; rb = t; }   // hook the larger root under the smaller
        const uint32_t seen = atomicCAS(&parent[ra], ra, rb);
        if (seen == ra) return true;
        ra = cc_find(parent, seen);   // ra was no longer a root: continue from what it points to now
        rb = cc_find(parent, rb);
    }
    return false;
}
// Island labels are maintained incrementally, and the HOST picks the mode from counters it fetched with the pair count:
//   CC_SKIP         unchanged pair set (in-place step): nothing is launched;
//   CC_INCREMENTAL  no island can have split: start from last step's labels (roots = a depth-1 forest), hook the new edges;
//   CC_FULL         recompute over all joints and manifolds (scene edits, or a certificate manifold disappeared).
// "No island can have split" is decided with a CERTIFICATE: every union the forest ever performed was made on a particular
// edge - a joint, or a manifold, which is then marked (Manifolds::tree). The marked edges form a spanning forest of the
// contact graph, so as long as every marked manifold of the previous array is still in this step's pair set
// (Counters::tree_found == tree_total, counted by k_bp_pairs while it re-tests the existing pairs) the components are intact,
// whatever other pairs went away. Manifolds that carry contact points are hooked first and separated AABBs almost always
// belong to manifolds without points, so on a settled pile the full recompute (~100 us: its cost is the depth of the
// initial forest) went from most steps to almost none. (Round 2 recomputed whenever ANY pair disappeared.)
enum { CC_SKIP = 0, CC_INCREMENTAL = 1, CC_FULL = 2 };
DI void cc_count_marks(uint32_t marks, Counters *cnt) {   // every lane of the wave calls this
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) marks += __shfl_xor(marks, off);
    if ((threadIdx.x & 63) == 0 && marks) atomicAdd(&cnt->tree_marks, marks);
}
// CC_FULL only: every body starts at its smallest dynamic lower-index neighbour it has CONTACT POINTS with (its manifolds
// with lower-index partners are the contiguous segment [seg_start, seg_end) of the sorted array). Links point to smaller
// indices, so this is a valid forest and most unions below find their roots already merged. Clears the segment's marks.
// (Round 6, built, measured and withdrawn - profiles/r06_tree_repair_experiment/, the patch is kept there: LOCAL REPAIR of the certificate. k_bp_pairs
//  listed the marked manifolds the new pair set drops, an extra workgroup of k_bp_compact looked for a replacement path a - c - b over manifolds
//  that exist in both arrays (c among a's lower-index partners) and marked it, the host then kept the incremental mode. Bit-exact, but a step
//  drops SEVERAL certificate manifolds and every one needs its path: 8 of 135 relabelling steps repaired on the headline pile, 20 of 384 on
//  mixed32k, 13 of 129 on islands256k, none on the polyhedron heap, which paid 4 % for the listing. EDYNHIP_TREE_STATS=1 prints the counts.)
// (Round 6, measured and dropped: offering the edges in classes of decreasing STABILITY - manifolds whose oldest point has lived for 32 steps,
//  then the other manifolds with points, then the pointless ones - so that the certificate consists of long-lived contacts. The number of
//  steps that relabel in full did not move (mixed32k 372 against 373 of 440, pile32k 127 / 128, islands256k 277 / 277, the polyhedron heap
//  every step either way) and the two kernels got slower (k_cc_hook_bodies 55 -> 70 us): what breaks a certificate on these scenes is not
//  a young contact flickering but some long-lived pair of 32 768 bodies separating, in nearly every step. DESIGN section 9, the round-6 list.)
__global__ void k_cc_init(uint32_t n, uint32_t *forest, Counters *cnt, Manifolds mf, uint32_t M, const uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) cnt->num_islands = 0;
    uint32_t marks = 0;
    if (i < n) {
        uint32_t parent = i;
        if (M && is_dynamic(flags[i])) {
            for (uint32_t s = mf.seg_start[i], e = mf.seg_end[i]; s < e; ++s) {
                const uint32_t lo = (uint32_t)(mf.skey[s] >> 1);
                uint8_t mark = 0;
                if (parent == i && (mf.info[s] & 0xFF) != 0 && is_dynamic(flags[lo])) { parent = lo; mark = 1; marks = 1; }
                mf.tree[s] = mark;
            }
        }
        forest[i] = parent;
    }
    cc_count_marks(marks, cnt);
}
// CC_FULL, between the initial forest and the unions (round 5): every body's link goes straight to its root. The initial forest of a pile
// is a set of chains ~100 links deep (each body under its lowest lower-index partner); without this pass every union of k_cc_hook_bodies
// walks such a chain twice. The walks halve the paths they pass, so a second pass costs little where the first has been.
__global__ void k_cc_compress(uint32_t n, uint32_t *forest, const uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && is_dynamic(flags[i])) forest[i] = cc_find(forest, i);   // (a racing hook cannot exist here: only finds run in this launch)
}
__global__ void k_cc_hook(uint32_t M, const uint32_t *__restrict__ bA, const uint32_t *__restrict__ bB,
                          const uint32_t *__restrict__ flags, uint32_t *island) {   // joints (CC_FULL): edges that only an edit removes
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M) return;
    uint32_t a = bA[e], b = bB[e];
    if (is_dynamic(flags[a]) && is_dynamic(flags[b])) (void)cc_union(island, a, b);
}
// Vertex-centric hooking for the full recompute: one lane per body walks the contiguous run of manifolds in which it
// is the higher-index partner. All unions of one body are issued by one lane in sequence, so lanes do not fight over
// the same root the way one-lane-per-edge does when a body has 6-12 partners. Manifolds with contact points first.
__global__ void k_cc_hook_bodies(uint32_t n, Manifolds mf, uint32_t M, const uint32_t *__restrict__ flags, uint32_t *island, Counters *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t marks = 0;
    if (i < n && M != 0 && is_dynamic(flags[i])) {
        const uint32_t s0 = mf.seg_start[i], s1 = mf.seg_end[i];
        auto hook = [&](uint32_t s) {
            const uint32_t lo = (uint32_t)(mf.skey[s] >> 1);
            if (!is_dynamic(flags[lo])) return;
            if (island[i] == island[lo]) return;   // both under the same node: one tree already (two loads instead of two walks; most edges of a pile end here)
            if (cc_union(island, i, lo)) { mf.tree[s] = 1; ++marks; }
        };
        // the manifolds with contact points first; the others are remembered (a bit each: an owner keeps at most kOwnCap = 64 in its segment,
        // longer segments take the plain second pass) and visited afterwards without reading the point counts again
        uint64_t later = 0;
        const bool fits = s1 - s0 <= 64u;
        for (uint32_t s = s0; s < s1; ++s) {
            if ((mf.info[s] & 0xFF) != 0) hook(s);
            else if (fits) later |= 1ull << (s - s0);
        }
        if (fits) for (; later; later &= later - 1) hook(s0 + (uint32_t)__ffsll((long long)later) - 1u);
        else for (uint32_t s = s0; s < s1; ++s) if ((mf.info[s] & 0xFF) == 0) hook(s);
    }
    cc_count_marks(marks, cnt);
}
__global__ void k_cc_hook_new(const uint2 *__restrict__ edges, const uint32_t *__restrict__ edge_m, uint8_t *tree, const uint32_t *__restrict__ flags,
                              uint32_t *island, Counters *cnt) {   // CC_INCREMENTAL: `island` holds last step's labels
    const uint32_t n = cnt->num_new;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->num_islands = 0;
    uint32_t marks = 0;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        uint2 ed = edges[e];
        if (is_dynamic(flags[ed.x]) && is_dynamic(flags[ed.y]) && cc_union(island, ed.x, ed.y)) { tree[edge_m[e]] = 1; ++marks; }
    }
    cc_count_marks(marks, cnt);
}
enum { SL_FAST = 1, SL_DISABLED = 2, SL_HAS_ASLEEP = 4, SL_HAS_AWAKE = 8, SL_WAKE = 16, SL_SPLIT = 32 };   // island state bits (k_sleep_*)
enum { SLA_KEEP = 0, SLA_AWAKE = 1, SLA_SLEEP = 2 };
// split_state (island sleeping, full relabel only): a body whose root differs from the root of last step's root of its island is a
// part of an island that fell apart - both parts are marked, k_sleep_decide starts their timers again (split_islands,
// island_manager.cpp:411-447: every part of a split island ends up with an empty sleep_timestamp).
template <bool BEGIN>
__global__ void k_cc_flatten(uint32_t n, const uint32_t *__restrict__ flags, uint32_t *island, uint32_t *label, Counters *cnt, int mode, Bodies b, float dt, uint32_t *first_slot,
                             uint32_t *split_state) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) cnt->tree_total = (mode == CC_FULL ? 0u : cnt->tree_total) + cnt->tree_marks;   // the hooks are done (kernel boundary)
    uint32_t root = 0;
    if (i < n) {
        uint32_t r = cc_find(island, i);
        if (split_state && is_dynamic(flags[i]) && !(flags[i] & BF_REMOVED)) {
            const uint32_t o = label[i];   // last step's root of this body's island (a full relabel works on a scratch forest: `label` is still last step's here)
            if (o < n && is_dynamic(flags[o]) && !(flags[o] & BF_REMOVED)) {
                const uint32_t ro = cc_find(island, o);
                if (ro != r) { atomicOr(&split_state[r], (uint32_t)SL_SPLIT); atomicOr(&split_state[ro], (uint32_t)SL_SPLIT); }
            }
        }
        label[i] = r;
        root = (r == i && is_dynamic(flags[i])) ? 1u : 0u;
        if (BEGIN) solve_begin_body(i, b, dt, first_slot);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) root += __shfl_xor(root, off);
    if ((threadIdx.x & 63) == 0 && root) atomicAdd(&cnt->num_islands, root);
}

// ------------------------------------------------------------------ island sleeping (island_manager.cpp:524-623)
// Islands are identified by their label (lowest body index). Per step, after the labels: (1) reduce every island's
// bodies into state bits, (2) mark the islands that received a manifold created this step, (3) one lane per island
// decides - wake (new edge, or sleeping and awake bodies merged), keep sleeping, run / restart the timer, go to sleep
// once the timer has run for more than island_time_to_sleep (measured on the step time stamps, ctx.hpp sim_clock) - (4) every body applies its island's decision (put_to_sleep zeroes velocities).
// merge_islands (island_manager.cpp:297-350): the BIGGEST of the islands that merge - nodes + edges - survives with its sleep timer.
// Labels are lowest body indices, so the surviving timer is carried to the merged island's label: per new island, the timer of the biggest
// of last step's islands it consists of; size = its procedural bodies + the edges it had before this step (manifolds that persist from
// the previous array, joints that existed at the last update), ties: the lowest old label (the checker's coloured order counts the same; pinned to the engine by
// tests/test_reference_engine.py::test_island_merge_keeps_the_bigger_islands_sleep_timer_like_the_real_engine). Three small passes
// in the steps of a world with island sleeping that relabel: k_sleep_sizes (sizes of last step's islands, keyed by last step's labels -
// a copy taken before the hooks, the union-find halves paths in place), the candidate maximum in k_sleep_scan, k_sleep_carry.
struct SleepMerge { const uint32_t *old_label; uint32_t prev_n; uint32_t prev_joints; uint32_t *size; unsigned long long *best; double *carried; };
DI void add_by_label(uint32_t label, uint32_t amount, uint32_t *dst) {   // every lane of the wave calls this (amount 0 = nothing): one atomic per distinct label and wave
    uint64_t todo = __ballot(amount != 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t l = (uint32_t)__shfl((int)label, leader);
        const bool mine = amount != 0 && label == l;
        uint32_t sum = mine ? amount : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&dst[l], sum);
        todo &= ~__ballot(mine);
    }
}
DI void or_by_label(uint32_t label, uint32_t bits, uint32_t *dst) {   // every lane of the wave calls this (bits 0 = nothing): one atomic per distinct label and wave
    // (one lane per body OR-ing into its island's word serialises on that word: a 32k-body pile - one island - spent 0.4 ms per step here)
    uint64_t todo = __ballot(bits != 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t l = (uint32_t)__shfl((int)label, leader);
        const bool mine = bits != 0 && label == l;
        uint32_t all = mine ? bits : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) all |= (uint32_t)__shfl_xor((int)all, off);
        // the word only gains bits while this kernel runs (k_sleep_decide zeroed it): a stale read can cost a redundant atomic, never a lost bit
        if ((int)(threadIdx.x & 63) == leader && (__hip_atomic_load(&dst[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & all) != all) atomicOr(&dst[l], all);
        todo &= ~__ballot(mine);
    }
}
__global__ void k_sleep_sizes(uint32_t n, Bodies b, Manifolds mf, uint32_t M, Joints j, SleepMerge sm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t label = 0, amount = 0;
    if (i < n && i < sm.prev_n && is_dynamic(b.flags[i]) && !(b.flags[i] & BF_REMOVED)) {
        label = sm.old_label[i];
        amount = 1;
        if (M) for (uint32_t s = mf.seg_start[i], e = mf.seg_end[i]; s < e; ++s) amount += mf.prev_idx[s] != 0xFFFFFFFFu ? 1u : 0u;   // this body's manifolds (it is their owner) that existed before this step
        if (label >= n) amount = 0;
    }
    add_by_label(label, amount, sm.size);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < j.n; e += gridDim.x * blockDim.x) {   // joints (few): plain atomics
        const uint32_t a = j.bodyA[e], bb = j.bodyB[e], x = is_dynamic(b.flags[a]) ? a : bb;
        if (j.orig[e] >= sm.prev_joints) continue;   // made since the last update: a new edge, in no island yet (merge_islands sizes the islands before it inserts them)
        if (x < sm.prev_n && is_dynamic(b.flags[x]) && sm.old_label[x] < n) atomicAdd(&sm.size[sm.old_label[x]], 1u);
    }
}
__global__ void k_sleep_carry(uint32_t n, Bodies b, SleepMerge sm, const double *__restrict__ since) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = sm.best[i];
    sm.best[i] = 0ull; sm.size[i] = 0u;   // armed for the next relabelling step
    sm.carried[i] = key ? since[~(uint32_t)key] : -1.0;
}
__global__ void k_sleep_scan(uint32_t n, Bodies b, uint32_t *state, SleepMerge sm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t label = 0, bits = 0;
    if (i < n) {
        const uint32_t fl = b.flags[i];
        if (is_dynamic(fl)) {
            label = b.island[i];
            // one of last step's island roots: a candidate for the timer of the island it is in now
            if (sm.best && i < sm.prev_n && !(fl & BF_REMOVED) && sm.old_label[i] == i)
                atomicMax(&sm.best[label], ((unsigned long long)sm.size[i] << 32) | (unsigned long long)(~i));
            const f3 v = from4(b.linvel[i]), w = from4(b.angvel[i]);
            const float lin = 0.005f, ang = 3.1415926535897932384626433832795029f / 48.0f;   // config/constants.hpp:41-42
            bits = (fl & BF_ASLEEP) ? SL_HAS_ASLEEP : SL_HAS_AWAKE;
            if (length_sqr(v) > lin * lin || length_sqr(w) > ang * ang) bits |= SL_FAST;
            if (fl & BF_NOSLEEP) bits |= SL_DISABLED;
        }
    }
    or_by_label(label, bits, state);
}
__global__ void k_sleep_edges(const uint2 *__restrict__ edges, const Counters *cnt, const uint32_t *__restrict__ label, uint32_t *state) {
    const uint32_t n = cnt->num_new;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x)
        atomicOr(&state[label[edges[e].x]], (uint32_t)SL_WAKE);   // .x = the pair's owner: always procedural
}
__global__ void k_sleep_decide(uint32_t n, Bodies b, uint32_t *state, uint32_t *action, double *since, double now, const double *__restrict__ carried) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = state[i];
    state[i] = 0;
    if (!is_dynamic(b.flags[i]) || b.island[i] != i) { since[i] = -1.0; return; }
    if (carried) since[i] = carried[i];   // a relabelling step: the timer of the biggest island this one is made of (k_sleep_carry)
    if (s & SL_SPLIT) since[i] = -1.0;   // a part of an island that split: the timer starts again
    const bool wake = (s & SL_WAKE) || ((s & SL_HAS_ASLEEP) && (s & SL_HAS_AWAKE));
    if ((s & SL_HAS_ASLEEP) && !(s & SL_HAS_AWAKE) && !wake) { action[i] = SLA_KEEP; return; }
    uint32_t a = SLA_AWAKE;
    if (!(s & SL_DISABLED) && !(s & SL_FAST)) {
        const double t0 = since[i];
        if (!(t0 >= 0.0)) since[i] = now;                                    // not running (a negative value or the all-ones fill)
        else if (now - t0 > 2.0) { a = SLA_SLEEP; since[i] = -1.0; }         // island_time_to_sleep, constants.hpp:48
    } else since[i] = -1.0;
    action[i] = a;
}
__global__ void k_sleep_apply(uint32_t n, Bodies b, const uint32_t *__restrict__ action, Counters *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t awake = 0;
    if (i < n) {
        uint32_t fl = b.flags[i];
        if (is_dynamic(fl)) {
            const uint32_t a = action[b.island[i]];
            if (a == SLA_AWAKE) { if (fl & BF_ASLEEP) { fl &= ~BF_ASLEEP; b.flags[i] = fl; } }
            else if (a == SLA_SLEEP) {
                fl |= BF_ASLEEP; b.flags[i] = fl;
                b.linvel[i] = make_float4(0, 0, 0, 0); b.angvel[i] = make_float4(0, 0, 0, 0);
            }
            awake = (fl & BF_ASLEEP) ? 0u : 1u;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) awake += __shfl_xor(awake, off);
    if ((threadIdx.x & 63) == 0 && awake) atomicAdd(&cnt->num_awake, awake);
}

int islands(edynhip_ctx *c) {
    hipStream_t s = c->stream;
    const uint32_t n = c->b.n, M = c->num_manifolds;
    if (n == 0) return EDYNHIP_OK;
    const Manifolds &mf = c->m[c->cur];
    const bool sleeping = c->sleep_active();   // (a world in which no body can sleep runs no sleep kernels: ctx.hpp num_sleepable)
    c->island_labels_valid = true;
    // union-find forest lives in isl_done (scratch until the position solver) to keep b.island stable for readers
    uint32_t *forest = c->isl_done;
    c->solve_begin_done = false;
    const uint32_t force = c->force_islands ? 1u : 0u;
    const uint32_t pm = c->prev_num_manifolds;
    c->force_islands = false;
    // No manifold now or in the previous step, nothing edited, no sleep decisions to take: the labels stand and every kernel below would
    // return at once - not launched at all (a world of joints only: 4 of its ~20 launches per step)
    if (!force && M == 0 && pm == 0 && !sleeping && c->full_step) return EDYNHIP_OK;
    // An in-place step (broadphase.hip: the pair set is last step's) has nothing to relabel. Otherwise the counters fetched with
    // the pair count say whether every certificate manifold is still there (see CC_INCREMENTAL above).
    const bool inplace = c->inplace_step;
    c->inplace_step = false;
    const int mode = force ? CC_FULL : inplace ? CC_SKIP
                     : (c->full_step && c->cnt_host->tree_found == c->cnt_host->tree_total) ? CC_INCREMENTAL : CC_FULL;
    (void)pm;
    if (mode == CC_FULL) ++c->cc_full_steps; else if (mode == CC_INCREMENTAL) ++c->cc_incremental_steps;
    // island sleeping: last step's labels, before the hooks rewrite them (the merge rule of k_sleep_sizes / k_sleep_carry reads them)
    if (sleeping && mode != CC_SKIP && c->sleep_old_label)
        EH_HIP(c, hipMemcpyAsync(c->sleep_old_label, c->b.island, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    // the solve's per-body start rides on the flatten kernel when nothing in between looks at velocities or sleep flags
    const bool begin = c->full_step && !sleeping && !c->has_restitution;
    auto flatten = [&](uint32_t *forest_or_labels) {
        uint32_t *split = (sleeping && mode == CC_FULL) ? c->sleep_state : nullptr;
        if (begin) hipLaunchKernelGGL(k_cc_flatten<true>, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b.flags, forest_or_labels, c->b.island, c->cnt, mode, c->b, c->cfg.fixed_dt, c->rows.first_slot, split);
        else hipLaunchKernelGGL(k_cc_flatten<false>, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b.flags, forest_or_labels, c->b.island, c->cnt, mode, c->b, c->cfg.fixed_dt, c->rows.first_slot, split);
        c->solve_begin_done = begin;
    };
    if (mode == CC_FULL) {
        hipLaunchKernelGGL(k_cc_init, dim3(blocks(n, 256)), dim3(256), 0, s, n, forest, c->cnt, mf, M, c->b.flags);
        if (c->j.n) hipLaunchKernelGGL(k_cc_hook, dim3(blocks(c->j.n, 256)), dim3(256), 0, s, c->j.n, c->j.bodyA, c->j.bodyB, c->b.flags, forest);
        const int compress_env = (int)c->knobs.cc_compress;   // developer knob: passes of k_cc_compress (the path bit: only where the step itself found the certificate broken)
        if (M && !force) c->paths |= compress_env <= 0 ? EDYNHIP_PATH_RELABEL_COMPRESS0 : compress_env == 1 ? EDYNHIP_PATH_RELABEL_COMPRESS1 : EDYNHIP_PATH_RELABEL_COMPRESSN;
        if (M) for (int pass = 0; pass < compress_env; ++pass) hipLaunchKernelGGL(k_cc_compress, dim3(blocks(n, 256)), dim3(256), 0, s, n, forest, c->b.flags);
        // (round 5, measured and dropped: one lane per EDGE on the compressed forest instead of the per-body walks - 2 x 67 us against 57:
        //  what costs is not the depth of the finds any more but the unions themselves, thousands of trees hooking into one root)
        if (M) hipLaunchKernelGGL(k_cc_hook_bodies, dim3(blocks(n, 256)), dim3(256), 0, s, n, mf, M, c->b.flags, forest, c->cnt);
        flatten(forest);
    } else if (mode == CC_INCREMENTAL) {   // the labels themselves are the forest (roots = lowest index: depth 1)
        hipLaunchKernelGGL(k_cc_hook_new, dim3(32), dim3(256), 0, s, c->new_edges, c->new_edge_m, mf.tree, c->b.flags, c->b.island, c->cnt);
        flatten(c->b.island);
    }
    if (sleeping) {
        const bool relabelled = mode != CC_SKIP && c->sleep_old_label != nullptr;
        SleepMerge sm{c->sleep_old_label, c->sleep_prev_n, c->sleep_prev_joints, c->sleep_size, c->sleep_best, c->sleep_carried};
        if (!relabelled) sm.best = nullptr;
        if (relabelled) hipLaunchKernelGGL(k_sleep_sizes, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b, mf, M, c->j, sm);
        hipLaunchKernelGGL(k_sleep_scan, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b, c->sleep_state, sm);
        if (relabelled) hipLaunchKernelGGL(k_sleep_carry, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b, sm, c->sleep_since);
        c->sleep_prev_n = n;
        c->sleep_prev_joints = (uint32_t)c->host_joints.size();
        hipLaunchKernelGGL(k_sleep_edges, dim3(32), dim3(256), 0, s, c->new_edges, c->cnt, c->b.island, c->sleep_state);
        hipLaunchKernelGGL(k_sleep_decide, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b, c->sleep_state, c->sleep_action, c->sleep_since, c->sim_clock,
                           relabelled ? c->sleep_carried : (const double *)nullptr);
        hipLaunchKernelGGL(k_sleep_apply, dim3(blocks(n, 256)), dim3(256), 0, s, n, c->b, c->sleep_action, c->cnt);
    }
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

}  // namespace eh
