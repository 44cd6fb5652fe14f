// What keeps the partition of the multi-device world (multi.hpp) valid: the monitor kernels - per step how far a body's AABB has grown out
// of the one recorded at the last check, per check the island boxes - the approach check on those boxes, and the re-partition, full or
// sticky, with what the islands carry through it. Also the host entry points of the partition rules (world_rules.hpp).
#include "multi.hpp"

namespace eh {

// ------------------------------------------------------------------------------------------------ device pieces
__device__ __forceinline__ uint32_t ordered_bits(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ inline float from_ordered_bits(uint32_t u) {
    const uint32_t v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f; memcpy(&f, &v, 4); return f;
}
__device__ __forceinline__ bool shard_body_counts(uint32_t fl) { return (fl & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC && !(fl & BF_REMOVED) && (fl & BF_SHAPE_MASK) != 0; }

// (b) above: the largest distance by which a dynamic body's AABB sticks out of the AABB recorded at the last check (0 = nothing moved out)
__global__ void k_shard_growth(uint32_t n, Bodies b, const float4 *__restrict__ amin0, const float4 *__restrict__ amax0, uint32_t *out_bits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float g = 0.0f;
    if (i < n && shard_body_counts(b.flags[i])) {
        const float4 lo = b.amin[i], hi = b.amax[i], lo0 = amin0[i], hi0 = amax0[i];
        g = fmaxf(fmaxf(fmaxf(lo0.x - lo.x, lo0.y - lo.y), lo0.z - lo.z), fmaxf(fmaxf(hi.x - hi0.x, hi.y - hi0.y), hi.z - hi0.z));
        g = fmaxf(g, 0.0f);
        if (!(g == g)) g = 3.0e38f;   // a NaN box: force a check (and let the check fail loudly)
    }
    for (int off = 32; off > 0; off >>= 1) g = fmaxf(g, __shfl_xor(g, off));
    if ((threadIdx.x & 63) == 0 && g > 0.0f) atomicMax(out_bits, __float_as_uint(g));   // non-negative floats order like their bits
}
__global__ void k_island_box_clear(uint32_t n, uint32_t *lo, uint32_t *hi) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * n) { lo[i] = 0xFFFFFFFFu; hi[i] = 0u; }
}
// (a) above, also records the boxes the growth is measured against
__global__ void k_island_box_reduce(uint32_t n, Bodies b, uint32_t *lo, uint32_t *hi, float4 *amin0, float4 *amax0, bool per_body) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 mn = b.amin[i], mx = b.amax[i];
    amin0[i] = mn; amax0[i] = mx;
    if (!shard_body_counts(b.flags[i])) return;
    uint32_t l = per_body ? i : b.island[i];
    if (l >= n) l = i;
    atomicMin(&lo[3 * l], ordered_bits(mn.x)); atomicMin(&lo[3 * l + 1], ordered_bits(mn.y)); atomicMin(&lo[3 * l + 2], ordered_bits(mn.z));
    atomicMax(&hi[3 * l], ordered_bits(mx.x)); atomicMax(&hi[3 * l + 1], ordered_bits(mx.y)); atomicMax(&hi[3 * l + 2], ordered_bits(mx.z));
}
__global__ void k_island_box_compact(uint32_t n, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint32_t *count, uint32_t *out_label, float *out_box) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n || lo[3 * l] == 0xFFFFFFFFu) return;   // no shaped dynamic body carries this label
    const uint32_t k = atomicAdd(count, 1u);
    out_label[k] = l;
    for (int d = 0; d < 3; ++d) { out_box[6 * k + d] = from_ordered_bits(lo[3 * l + d]); out_box[6 * k + 3 + d] = from_ordered_bits(hi[3 * l + d]); }
}

}  // namespace eh

using namespace eh;
using namespace eh::world;

namespace {

// the three island-box kernels over the monitor scratch `d` of n bodies (k_island_box_*), behind a clear of the growth bits and the count
hipError_t launch_island_boxes(hipStream_t st, uint32_t n, const Bodies &b, uint32_t *d, const MonLayout &L, bool per_body) {
    const hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(uint32_t), st);
    hipLaunchKernelGGL(k_island_box_clear, dim3((3 * n + 255) / 256), dim3(256), 0, st, n, d + L.lo, d + L.hi);
    hipLaunchKernelGGL(k_island_box_reduce, dim3((n + 255) / 256), dim3(256), 0, st, n, b, d + L.lo, d + L.hi, (float4 *)(d + L.amin0), (float4 *)(d + L.amax0), per_body);
    hipLaunchKernelGGL(k_island_box_compact, dim3((n + 255) / 256), dim3(256), 0, st, n, d + L.lo, d + L.hi, d + 1, d + L.out_label, (float *)(d + L.out_box));
    return e;
}

// island boxes of shard r, reduced on its device; also records the AABBs the growth is measured against and clears the growth.
// per_body: every body is its own "island" (right after a shard was built its device labels are not computed yet; body boxes are
// the exact criterion anyway - island boxes are the cheaper, more conservative aggregate).
void island_boxes_shard(edynhip_world *w, uint32_t r, bool per_body) {
    Shard &s = w->shards[r];
    if (s.rc != EDYNHIP_OK) return;
    const uint32_t nl = (uint32_t)s.local_ids.size();
    s.res.mon_host[1] = 0;
    if (nl == 0) return;
    SH_HIP(s, hipSetDevice(s.device));
    hipStream_t st = s.ctx->stream;
    const MonLayout L(s.cap);
    uint32_t *d = s.res.mon_dev;
    SH_HIP(s, launch_island_boxes(st, nl, s.ctx->b, d, L, per_body));
    SH_HIP(s, hipMemcpyAsync(s.res.mon_host, d, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SH_HIP(s, hipStreamSynchronize(st));
    const uint32_t k = s.res.mon_host[1];
    if (k) {
        SH_HIP(s, hipMemcpyAsync(s.res.mon_host + 2, d + L.out_label, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SH_HIP(s, hipMemcpyAsync(s.res.mon_host + 2 + s.cap, d + L.out_box, (size_t)k * 6 * sizeof(float), hipMemcpyDeviceToHost, st));
        SH_HIP(s, hipStreamSynchronize(st));
    }
}

// contact events: the ids of a collected shard's points go with the re-partition, by global body pair (before s.manifolds is taken apart)
void carry_point_ids(const Shard &s, Carry &carry) {
    if (s.pids.size() != 4 * s.manifolds.size()) return;
    for (size_t k = 0; k < s.manifolds.size(); ++k) {
        const edynhip_manifold &m = s.manifolds[k];
        std::array<uint64_t, 4> row;
        std::memcpy(row.data(), &s.pids[4 * k], sizeof(row));
        carry.point_ids[((uint64_t)s.local_ids[m.body[0]] << 32) | s.local_ids[m.body[1]]] = row;
    }
}

// materials: the extras rows of a collected shard's points go with the re-partition, by global body pair like the ids
void carry_point_extras(const Shard &s, Carry &carry) {
    if (s.manifolds.empty() || s.xrows != s.manifolds.size()) return;
    for (size_t k = 0; k < s.manifolds.size(); ++k) {
        const edynhip_manifold &m = s.manifolds[k];
        std::array<float, kExtrasRowFloats> row;
        std::memcpy(row.data(), s.res.xtr_host + kExtrasRowFloats * k, sizeof(row));   // (straight from the pinned rows the collect read)
        carry.point_extras[((uint64_t)s.local_ids[m.body[0]] << 32) | s.local_ids[m.body[1]]] = row;
    }
}

// the applied impulses and tracked angles of a collected shard's joints go with the re-partition, by global joint
void carry_joint_impulses(const Shard &s, Carry &carry) {
    for (uint32_t lj = 0; lj < s.local_joints.size() && !s.imp24.empty(); ++lj) {
        const uint32_t g = s.local_joints[lj];
        std::memcpy(&carry.imp24[(size_t)g * 24], &s.imp24[(size_t)lj * 24], 24 * sizeof(float));
        carry.angle[g] = s.imp10[(size_t)lj * 10 + 9];
    }
}

}  // namespace

namespace eh {
namespace world {

// The approach check on the device-reduced island boxes. Returns true when islands of different shards are within the creation
// margin of each other; otherwise w->budget = how far they may still approach.
int approach_check(edynhip_world *w, bool &close, bool per_body, const std::vector<IslandBox> *host_boxes) {
    w->pool->run([w, per_body](uint32_t r) { island_boxes_shard(w, r, per_body); });
    EH_TRY(shard_error(w));
    std::vector<IslandBox> boxes;
    if (host_boxes) {   // the caller knows the islands of this state (a re-partition): their boxes, owned by the shard their bodies went to
        boxes = *host_boxes;
        for (IslandBox &b : boxes) b.owner = b.label < w->rank_of.size() ? w->rank_of[b.label] : -1;
    } else
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        Shard &s = w->shards[r];
        const uint32_t k = s.local_ids.empty() ? 0 : s.res.mon_host[1];
        const float *bx = (const float *)(s.res.mon_host + 2 + s.cap);
        for (uint32_t q = 0; q < k; ++q) {
            const uint32_t lead = s.local_ids[s.res.mon_host[2 + q]];
            if (w->rank_of[lead] != (int32_t)r) continue;   // (cannot happen: replicated bodies are not dynamic)
            IslandBox b;
            for (int d = 0; d < 3; ++d) { b.lo[d] = bx[6 * q + d]; b.hi[d] = bx[6 * q + 3 + d]; }
            b.label = lead; b.owner = (int32_t)r;
            boxes.push_back(b);
        }
    }
    ++w->stats.approach_checks;
    approach_verdict(boxes, close, w->budget);
    return EDYNHIP_OK;
}

// `only` (or nullptr = all): the shards to build; the others keep their contexts - their bodies, and therefore their local indices, are unchanged.
int rebuild(edynhip_world *w, const Carry &carry, bool from_state, const std::vector<uint8_t> *only) {
    PhaseTrace trace(w, "rebuild");
    w->pool->run([&](uint32_t r) { if (!only || (*only)[r]) build_shard(w, r, carry, from_state); });
    EH_TRY(shard_error(w));
    trace.mark("build the shards (in parallel)");
    w->pool->run([w](uint32_t r) { gather_shard(w, r, false); });
    EH_TRY(shard_error(w));
    trace.mark("gather");
    refresh_bodies_per_shard(w);
    w->built = true;
    bool close = false;
    // a fresh partition keeps close islands together: the check sets the budget and records the reference boxes the growth is measured against
    const int rc_check = approach_check(w, close, true, carry.island_boxes.empty() ? nullptr : &carry.island_boxes);
    trace.mark(carry.island_boxes.empty() ? "approach check on body boxes" : "approach check (reference boxes on the devices, island boxes from the host)");
    return rc_check;
}

// Re-partition. FULL (edynhip_world_repartition, on request): everything the islands carry is read from every shard, the islands are
// balanced afresh (longest processing time first over their contact rows) and every shard is rebuilt. STICKY (the approach check found
// islands of different shards within the creation margin of each other - what a step does by itself): the islands stay where they are, a
// group of islands that has to live together moves to the shard that already holds most of it, and only the shards that gain or lose a
// body are read in full and rebuilt - the cost of an island meeting its neighbour follows the two shards involved, not the world
// (round 5: a collapsing 262 144-box scene re-partitioned 18 times in 160 steps at 8 s each when every meeting rebuilt all shards from an
// unrelated partition; scripts/multi_overhead.py).
// Edits of a running world come in with `edges` (body pairs that have to share a shard: a joint about to be made between two shards),
// `force` (shards to rebuild whatever moves: one that needs a larger context) and from_edit: no step may have run since a shard was
// built, so its device labels are not those of its islands - the labels it was built with stand in (the state has not moved since).
int repartition(edynhip_world *w, bool sticky, const std::vector<std::array<uint32_t, 2>> *edges, const std::vector<uint8_t> *force, bool from_edit) {
    const HostScene &sc = w->scene;
    const uint32_t n = sc.n, W = (uint32_t)w->shards.size();
    // A body removed since the last step is its own island by the device labels (k_mark_removed) while its manifolds still tie it to its
    // old one: only the full pass reads every manifold before it welds, so an edit that rebuilds shards in that state takes it (rare: a
    // removal and a rebuilding edit with no step in between)
    if (from_edit && !w->pending_tombs.empty()) sticky = false;
    PhaseTrace trace(w, sticky ? "sticky re-partition" : "full re-partition");
    w->pool->run([w, sticky](uint32_t r) { collect_shard(w, r, true, !sticky, w->carries_extras()); });
    EH_TRY(shard_error(w));
    trace.mark("collect light state of every shard");
    std::vector<uint32_t> labels(n);
    std::iota(labels.begin(), labels.end(), 0u);
    std::vector<float> aabb((size_t)n * 6, 0.f);
    std::vector<double> weights(n, 1.0);
    Carry carry;
    carry.any = true;
    if (sc.nj) { carry.imp24.assign((size_t)sc.nj * 24, 0.f); carry.angle.assign(sc.nj, 0.f); }
    if (w->cfg.flags & EDYNHIP_FLAG_SLEEPING) { carry.asleep.assign(n, 0); carry.label.resize(n); std::iota(carry.label.begin(), carry.label.end(), 0u); carry.since.assign(n, -1.0); }
    for (uint32_t r = 0; r < W; ++r) {
        Shard &s = w->shards[r];
        if (!carry.label.empty() && !s.local_ids.empty()) carry.clock = std::max(carry.clock, s.sleep_clock);   // (every shard has taken the same steps)
        for (uint32_t l = 0; l < s.local_ids.size(); ++l) {
            const uint32_t g = s.local_ids[l];
            if (w->rank_of[g] != (int32_t)r) continue;
            labels[g] = s.local_ids[s.labels[l]];
            std::memcpy(&aabb[6 * (size_t)g], &s.aabb[6 * (size_t)l], 24);
            if (!carry.asleep.empty()) carry.asleep[g] = s.asleep[l];
            if (!carry.label.empty() && s.sleep_label[l] < s.local_ids.size()) {
                carry.label[g] = s.local_ids[s.sleep_label[l]];
                if (s.sleep_label[l] == l) carry.since[g] = s.sleep_since[l];
            }
        }
    }
    if (from_edit)
        for (uint32_t r = 0; r < W; ++r) {
            const Shard &s = w->shards[r];
            if (!s.ctx || s.ctx->step_index != 0) continue;
            for (uint32_t g : s.local_ids) if (w->rank_of[g] == (int32_t)r) labels[g] = w->query_labels.size() == n ? w->query_labels[g] : g;
        }
    // the island query's labels: a shard that has not stepped since it was rebuilt still answers with the labels it was rebuilt with
    carry.island = labels;
    if (w->query_labels.size() == n)
        for (uint32_t r = 0; r < W; ++r) {
            const Shard &s = w->shards[r];
            if (!s.ctx || !s.ctx->query_island || s.ctx->step_index != 0) continue;
            for (uint32_t g : s.local_ids) if (w->rank_of[g] == (int32_t)r) carry.island[g] = w->query_labels[g];
        }
    w->query_labels = carry.island;
    // what travels with the bodies of the shards read in full (all of them / later: the ones that change)
    auto take_heavy = [&](const std::vector<uint8_t> *only) {
        for (uint32_t r = 0; r < W; ++r) {
            Shard &s = w->shards[r];
            if (only && !(*only)[r]) { s.manifolds.clear(); continue; }
            carry_point_ids(s, carry);
            carry_point_extras(s, carry);
            for (const edynhip_manifold &m : s.manifolds) {   // weight = 1 + the contact points the body takes part in (balance the rows)
                const uint32_t a = s.local_ids[m.body[0]], b = s.local_ids[m.body[1]];
                if (w->rank_of[a] == (int32_t)r) weights[a] += m.num_points;
                if (w->rank_of[b] == (int32_t)r) weights[b] += m.num_points;
            }
            carry_joint_impulses(s, carry);
        }
        merge_manifolds(w, carry.manifolds);
    };
    if (!sticky) take_heavy(nullptr);
    // The islands that must end up on one shard, welded (weld_islands): overlapping boxes, live joints, the edit's edges, carried
    // manifolds. (A sticky re-partition follows a step of every shard: labels are current, and it carries no manifold list.)
    std::vector<IslandBox> boxes;
    std::vector<EdgeSpan> tied;
    if (sc.nj) tied.push_back({sc.jbody.data(), 2 * sizeof(uint32_t), sc.nj, sc.jalive.data()});
    if (edges && !edges->empty()) tied.push_back({edges->data(), sizeof((*edges)[0]), edges->size(), nullptr});
    if (!carry.manifolds.empty()) tied.push_back({carry.manifolds[0].body, sizeof(edynhip_manifold), carry.manifolds.size(), nullptr});
    const std::vector<uint32_t> welded = weld_islands(n, labels.data(), sc.kind.data(), sc.shape_type.data(), aabb.data(), tied, boxes);
    ++w->stats.repartitions;
    trace.mark("island boxes, welding");
    if (!sticky) {
        if (!carry.point_extras.empty()) ++w->stats.extras_carries;
        w->rank_of.assign(n, -1);
        partition_islands_spatial(n, welded.data(), sc.kind.data(), weights.data(), aabb.data(), W, w->rank_of.data());
        return rebuild(w, carry, true);
    }
    const std::vector<int32_t> next = sticky_targets(n, welded.data(), sc.kind.data(), w->rank_of.data(), W);
    if (needs_rebalance(n, next.data(), W)) {   // this meeting takes the full, spatially balanced re-partition instead
        ++w->stats.rebalances; --w->stats.repartitions;   // (counted again by the full pass)
        return repartition(w, false, edges, nullptr, from_edit);
    }
    std::vector<uint8_t> changed(W, 0);
    for (uint32_t i = 0; i < n; ++i) if (next[i] != w->rank_of[i]) { changed[(uint32_t)next[i]] = 1; changed[(uint32_t)w->rank_of[i]] = 1; }
    if (force) for (uint32_t r = 0; r < W; ++r) if ((*force)[r]) changed[r] = 1;
    if (std::none_of(changed.begin(), changed.end(), [](uint8_t c) { return c != 0; })) {
        // nothing has to move (the close islands already share a shard): only the budget is taken again
        bool close = false;
        EH_TRY(approach_check(w, close, true));
        return EDYNHIP_OK;
    }
    trace.mark("sticky targets");
    w->pool->run([w, &changed](uint32_t r) { if (changed[r]) collect_shard(w, r, false, true, w->carries_extras()); });
    EH_TRY(shard_error(w));
    trace.mark("collect manifolds / joint impulses of the changed shards");
    for (uint32_t r = 0; r < W; ++r) if (changed[r]) { carry_point_ids(w->shards[r], carry); carry_point_extras(w->shards[r], carry); carry_joint_impulses(w->shards[r], carry); }
    // Manifolds: a body that stays in its shard keeps its place among the others that stay (local indices ascend with the global ones), so
    // the manifolds that stay ARE in canonical order already; only those whose island moves are taken out, sorted among themselves and
    // merged into their new shard's list. No global sort, one copy per record at most (the merged, sorted list of every changed shard's
    // manifolds was 0.1-0.3 s of a re-partition).
    std::vector<std::vector<edynhip_manifold>> leaving(W);
    w->pool->run([&](uint32_t q) {
        if (!changed[q]) return;
        Shard &s = w->shards[q];
        size_t keep = 0;
        for (size_t k = 0; k < s.manifolds.size(); ++k) {
            edynhip_manifold m = s.manifolds[k];
            m.body[0] = s.local_ids[m.body[0]]; m.body[1] = s.local_ids[m.body[1]];
            const uint32_t dyn = w->rank_of[m.body[0]] >= 0 ? m.body[0] : m.body[1];
            if (w->rank_of[dyn] != (int32_t)q) continue;          // (not this shard's to report: cannot happen - a manifold lives where its dynamic body does)
            if (next[dyn] == (int32_t)q) s.manifolds[keep++] = m; else leaving[q].push_back(m);
        }
        s.manifolds.resize(keep);
    });
    std::vector<std::vector<edynhip_manifold>> incoming(W);
    for (uint32_t q = 0; q < W; ++q)
        for (const edynhip_manifold &m : leaving[q]) {
            const uint32_t dyn = w->rank_of[m.body[0]] >= 0 ? m.body[0] : m.body[1];
            incoming[(uint32_t)next[dyn]].push_back(m);
        }
    carry.per_shard.assign(W, {});
    w->pool->run([&](uint32_t r) {
        if (!changed[r]) return;
        Shard &s = w->shards[r];
        auto key_less = [&](const edynhip_manifold &x, const edynhip_manifold &y) { return canonical_key(sc.kind.data(), x.body[0], x.body[1]) < canonical_key(sc.kind.data(), y.body[0], y.body[1]); };
        if (incoming[r].empty()) { carry.per_shard[r].swap(s.manifolds); return; }
        std::sort(incoming[r].begin(), incoming[r].end(), key_less);
        carry.per_shard[r].resize(s.manifolds.size() + incoming[r].size());
        std::merge(s.manifolds.begin(), s.manifolds.end(), incoming[r].begin(), incoming[r].end(), carry.per_shard[r].begin(), key_less);
        s.manifolds.clear(); s.manifolds.shrink_to_fit();
    });
    trace.mark("sort out the carried manifolds per new shard");
    if (!carry.point_extras.empty()) ++w->stats.extras_carries;
    carry.island_boxes = boxes;
    w->rank_of = next;
    const int rc_rebuild = rebuild(w, carry, true, &changed);
    trace.mark("rebuild changed shards (+ gather, approach check)");
    return rc_rebuild;
}

}  // namespace world
}  // namespace eh

extern "C" {

int edynhip_partition_islands(uint32_t n, const uint32_t *labels, const int32_t *kind, const double *weights, uint32_t world_size, int32_t *rank_of) {
    if ((n && (!labels || !kind || !rank_of)) || world_size == 0) return EDYNHIP_ERR_INVALID;
    partition_islands(n, labels, kind, weights, world_size, rank_of);
    return EDYNHIP_OK;
}

int edynhip_island_boxes_overlap(uint32_t num_islands, const float *boxes6, const uint32_t *labels, const int32_t *owner, float margin, int any_owner,
                                 uint32_t *pairs, uint32_t capacity, uint32_t *num_pairs) {
    if ((num_islands && (!boxes6 || !labels || !owner)) || !num_pairs) return EDYNHIP_ERR_INVALID;
    std::vector<IslandBox> boxes(num_islands);
    for (uint32_t k = 0; k < num_islands; ++k) {
        for (int d = 0; d < 3; ++d) { boxes[k].lo[d] = boxes6[6 * k + d]; boxes[k].hi[d] = boxes6[6 * k + 3 + d]; }
        boxes[k].label = labels[k]; boxes[k].owner = owner[k];
    }
    std::vector<std::pair<uint32_t, uint32_t>> hits;
    sweep_boxes(boxes, margin, !any_owner, [&](const IslandBox &a, const IslandBox &b, float) { hits.emplace_back(std::min(a.label, b.label), std::max(a.label, b.label)); });
    std::sort(hits.begin(), hits.end());
    hits.erase(std::unique(hits.begin(), hits.end()), hits.end());
    *num_pairs = (uint32_t)hits.size();
    if (pairs) {
        if (capacity < hits.size()) return EDYNHIP_ERR_CAPACITY;
        for (size_t k = 0; k < hits.size(); ++k) { pairs[2 * k] = hits[k].first; pairs[2 * k + 1] = hits[k].second; }
    }
    return EDYNHIP_OK;
}

int edynhip_get_island_boxes(edynhip_ctx *c, uint32_t *labels, float *boxes6, uint32_t capacity, uint32_t *num_islands) {
    if (!c || !num_islands) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    *num_islands = 0;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    const MonLayout L(n);
    DeviceBuf<uint32_t> scratch;
    EH_HIP(c, scratch.alloc(L.words));
    uint32_t *d = scratch;
    uint32_t *count = d + 1, *out_label = d + L.out_label;
    float *out_box = (float *)(d + L.out_box);
    hipError_t e = launch_island_boxes(c->stream, n, c->b, d, L, false);
    uint32_t k = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&k, count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int rc = EDYNHIP_OK;
    if (e == hipSuccess) {
        *num_islands = k;
        if (labels && boxes6) {
            if (capacity < k) rc = set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_island_boxes: capacity");
            else if (k) {
                e = hipMemcpyAsync(labels, out_label, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(boxes6, out_box, (size_t)k * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            }
        }
    }
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_get_island_boxes", e);
    return rc;
}

int edynhip_world_repartition(edynhip_world *w) {
    if (!w) return EDYNHIP_ERR_INVALID;
    EH_TRY(ensure_built(w));
    return repartition(w, false);
}

}  // extern "C"
