// Queries on the multi-device world (multi.hpp).
//
// Every shard answers for its own bodies with the single context's kernels (eh::shard_raycast / shard_query_*), on its pool thread and
// its context's stream; local indices become global ones on the shard's device; the answers meet on the home device (devices[0]),
// where world_query.hip merges them into what ONE context holding the whole scene returns. A shard on the home device reads the
// caller's arrays and writes its answer in place; any other shard's queries and answers travel device to device.
#include "multi.hpp"
#include "world_query.hpp"

using namespace eh;
using namespace eh::world;

namespace {

constexpr uint32_t kWorldChunk = 1u << 20;   // rays per pass (raycast.hip kChunk)
constexpr unsigned long long kSat32 = 0xFFFFFFFFull;

int query_begin(edynhip_world *w) {
    EH_TRY(ensure_built(w));
    W_HIP(w, hipSetDevice(w->devices[0]));
    if (!w->qstream) W_HIP(w, w->qstream.create(hipStreamNonBlocking));
    if (!w->q_pin) W_HIP(w, w->q_pin.alloc(2));
    return EDYNHIP_OK;
}

// the shards that hold bodies, and each one's slot among them
uint32_t active_slots(const edynhip_world *w, std::vector<int32_t> &slot) {
    uint32_t k = 0;
    slot.assign(w->shards.size(), -1);
    for (uint32_t r = 0; r < w->shards.size(); ++r) if (w->shards[r].ctx && !w->shards[r].local_ids.empty()) slot[r] = (int32_t)k++;
    return k;
}

// m <= kWorldChunk rays, arrays on the home device
int world_raycast_chunk(edynhip_world *w, uint32_t m, const float4 *p0, const float4 *p1, uint32_t num_ignore, const uint32_t *ignore, uint32_t flags, void *out) {
    const int home = w->devices[0];
    std::vector<int32_t> slot;
    const uint32_t A = active_slots(w, slot);
    W_HIP(w, hipSetDevice(home));
    W_HIP(w, w->h_hits.grow((size_t)std::max(A, 1u) * m * sizeof(edynhip_raycast_hit)));
    w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        if (slot[r] < 0 || s.rc != EDYNHIP_OK) return;
        SH_HIP(s, hipSetDevice(s.device));
        hipStream_t st = s.ctx->stream;
        const uint32_t nl = (uint32_t)s.local_ids.size();
        uint8_t *dst = (uint8_t *)w->h_hits.h + (size_t)slot[r] * m * sizeof(edynhip_raycast_hit);
        const void *a = p0, *b = p1;
        void *o = dst;
        if (s.device != home) {
            SH_HIP(s, s.res.q_in.grow(2 * (size_t)m * sizeof(float4)));
            SH_HIP(s, s.res.q_out.grow((size_t)m * sizeof(edynhip_raycast_hit)));
            SH_HIP(s, hipMemcpyPeerAsync(s.res.q_in.h, s.device, p0, home, (size_t)m * sizeof(float4), st));
            SH_HIP(s, hipMemcpyPeerAsync((float4 *)s.res.q_in.h + m, s.device, p1, home, (size_t)m * sizeof(float4), st));
            a = s.res.q_in.h; b = (const float4 *)s.res.q_in.h + m; o = s.res.q_out.h;
        }
        s.q_ignore.clear();
        for (uint32_t k = 0; k < num_ignore; ++k)
            if (ignore[k] < w->scene.n && s.to_local[ignore[k]] >= 0) s.q_ignore.push_back((uint32_t)s.to_local[ignore[k]]);
        SH_TRY(s, shard_raycast(s.ctx, m, a, b, (uint32_t)s.q_ignore.size(), s.q_ignore.data(), flags, o));
        wq_translate_hits(st, m, o, s.res.ids_dev, nl);
        SH_HIP(s, hipGetLastError());
        if (s.device != home) SH_HIP(s, hipMemcpyPeerAsync(dst, home, o, s.device, (size_t)m * sizeof(edynhip_raycast_hit), st));
        SH_HIP(s, hipStreamSynchronize(st));
    });
    EH_TRY(shard_error(w));
    W_HIP(w, hipSetDevice(home));
    wq_rc_merge(w->qstream, A, m, w->h_hits.h, m, out);
    W_HIP(w, hipGetLastError());
    W_HIP(w, hipStreamSynchronize(w->qstream));   // (the shards' answers are overwritten by the next pass)
    return EDYNHIP_OK;
}

// The count pass: offsets [n + 1] and total [1] on the home device; the 64-bit total in *tot. The shards keep their counts and lists for
// world_query_fill.
int world_query_count(edynhip_world *w, int category, uint32_t n, const float4 *boxes, uint32_t flags, uint32_t *offsets, uint32_t *total, unsigned long long *tot) {
    const int home = w->devices[0];
    std::vector<int32_t> slot;
    const uint32_t A = n ? active_slots(w, slot) : 0u;
    W_HIP(w, hipSetDevice(home));
    W_HIP(w, w->h_cnt.grow((size_t)std::max(A, 1u) * std::max(n, 1u) * sizeof(uint32_t)));
    if (A) w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        if (slot[r] < 0 || s.rc != EDYNHIP_OK) return;
        SH_HIP(s, hipSetDevice(s.device));
        hipStream_t st = s.ctx->stream;
        s.res.q_boxes = boxes;
        if (s.device != home) {
            SH_HIP(s, s.res.q_in.grow(2 * (size_t)n * sizeof(float4)));
            SH_HIP(s, hipMemcpyPeerAsync(s.res.q_in.h, s.device, boxes, home, 2 * (size_t)n * sizeof(float4), st));
            s.res.q_boxes = s.res.q_in.h;
        }
        const unsigned long long *t64 = nullptr;
        SH_TRY(s, shard_query_count(s.ctx, category, n, s.res.q_boxes, flags, &s.res.q_cnt, &s.res.q_off, &t64));
        SH_HIP(s, hipMemcpyAsync(s.res.q_tot, t64, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (s.device != home)
            SH_HIP(s, hipMemcpyPeerAsync((uint32_t *)w->h_cnt.h + (size_t)slot[r] * n, home, s.res.q_cnt, s.device, (size_t)n * sizeof(uint32_t), st));
        SH_HIP(s, hipStreamSynchronize(st));
    });
    EH_TRY(shard_error(w));
    WqShards sh{};
    sh.W = A;
    for (uint32_t r = 0; r < w->shards.size() && A; ++r)
        if (slot[r] >= 0) sh.cnt[slot[r]] = w->shards[r].device == home ? w->shards[r].res.q_cnt : (const uint32_t *)w->h_cnt.h + (size_t)slot[r] * n;
    W_HIP(w, hipSetDevice(home));
    const size_t nb = (size_t)n / 256 + 2;   // scratch: total | block sums | their scan | summed counts
    W_HIP(w, w->h_scan.grow((1 + 2 * nb) * sizeof(unsigned long long) + (size_t)std::max(n, 1u) * sizeof(uint32_t)));
    unsigned long long *t64 = (unsigned long long *)w->h_scan.h, *bsum = t64 + 1, *boff = bsum + nb;
    wq_qa_offsets(w->qstream, sh, n, (uint32_t *)(boff + nb), bsum, boff, t64, offsets, total);
    W_HIP(w, hipGetLastError());
    W_HIP(w, hipMemcpyAsync(w->q_pin, t64, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    *tot = w->q_pin[0];
    return EDYNHIP_OK;
}

// The fill pass of the queries counted last: ids [capacity] on the home device; nothing is written at or beyond capacity.
int world_query_fill(edynhip_world *w, int category, uint32_t n, uint32_t flags, const uint32_t *offsets, uint32_t *ids, uint32_t capacity) {
    const int home = w->devices[0];
    std::vector<int32_t> slot;
    const uint32_t A = active_slots(w, slot);
    if (n == 0 || A == 0 || capacity == 0) return EDYNHIP_OK;
    // a shard's own list is sized by its own total: it must be addressable with 32 bits
    std::vector<size_t> base(w->shards.size(), 0);
    size_t remote_ids = 0;
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        if (slot[r] < 0) continue;
        if (*w->shards[r].res.q_tot >= kSat32) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_query_aabb: a shard reports 2^32 - 1 hits or more");
        if (w->shards[r].device != home) { base[r] = remote_ids; remote_ids += (size_t)*w->shards[r].res.q_tot; }
    }
    W_HIP(w, hipSetDevice(home));
    W_HIP(w, w->h_ids.grow(std::max<size_t>(remote_ids, 1) * sizeof(uint32_t)));
    W_HIP(w, w->h_off.grow((size_t)A * ((size_t)n + 1) * sizeof(uint32_t)));
    w->pool->run([&](uint32_t r) {
        Shard &s = w->shards[r];
        if (slot[r] < 0 || s.rc != EDYNHIP_OK) return;
        SH_HIP(s, hipSetDevice(s.device));
        hipStream_t st = s.ctx->stream;
        const size_t t = (size_t)*s.res.q_tot;
        if (t == 0 && s.device == home) return;
        SH_HIP(s, s.res.q_ids.grow(std::max<size_t>(t, 1) * sizeof(uint32_t)));
        SH_TRY(s, shard_query_fill(s.ctx, category, n, s.res.q_boxes, flags, (uint32_t *)s.res.q_ids.h, (uint32_t)t));
        wq_translate_ids(st, (uint32_t *)s.res.q_ids.h, t, s.res.ids_dev, (uint32_t)s.local_ids.size());   // (island labels are body indices too)
        SH_HIP(s, hipGetLastError());
        if (s.device != home) {
            SH_HIP(s, hipMemcpyPeerAsync((uint32_t *)w->h_off.h + (size_t)slot[r] * ((size_t)n + 1), home, s.res.q_off, s.device, ((size_t)n + 1) * sizeof(uint32_t), st));
            if (t) SH_HIP(s, hipMemcpyPeerAsync((uint32_t *)w->h_ids.h + base[r], home, s.res.q_ids.h, s.device, t * sizeof(uint32_t), st));
        }
        SH_HIP(s, hipStreamSynchronize(st));
    });
    EH_TRY(shard_error(w));
    WqShards sh{};
    sh.W = A;
    for (uint32_t r = 0; r < w->shards.size(); ++r) {
        if (slot[r] < 0) continue;
        const Shard &s = w->shards[r];
        const bool here = s.device == home;
        sh.off[slot[r]] = here ? s.res.q_off : (const uint32_t *)w->h_off.h + (size_t)slot[r] * ((size_t)n + 1);
        sh.ids[slot[r]] = here ? (const uint32_t *)s.res.q_ids.h : (const uint32_t *)w->h_ids.h + base[r];
    }
    W_HIP(w, hipSetDevice(home));
    for (uint32_t r = 0; r < w->shards.size(); ++r)
        if (slot[r] >= 0) wq_qa_merge(w->qstream, sh, (uint32_t)slot[r], n, (uint32_t)*w->shards[r].res.q_tot, offsets, ids, capacity);
    W_HIP(w, hipGetLastError());
    W_HIP(w, hipStreamSynchronize(w->qstream));
    return EDYNHIP_OK;
}

int check_world_query(edynhip_world *w, int category, uint32_t flags, const char *who) {
    if (category != EDYNHIP_QUERY_PROCEDURAL && category != EDYNHIP_QUERY_NON_PROCEDURAL && category != EDYNHIP_QUERY_ISLANDS)
        return w->fail(EDYNHIP_ERR_INVALID, std::string(who) + ": unknown category");
    if (flags & ~(uint32_t)EDYNHIP_QUERY_BRUTE_FORCE) return w->fail(EDYNHIP_ERR_INVALID, std::string(who) + ": unknown flag bits");
    return EDYNHIP_OK;
}

}  // namespace

extern "C" {

int edynhip_world_raycast_device(edynhip_world *w, uint32_t n, const void *p0_f4, const void *p1_f4, uint32_t num_ignore, const uint32_t *ignore,
                                 uint32_t flags, void *out) {
    if (!w || (n && (!p0_f4 || !p1_f4 || !out)) || (num_ignore && !ignore)) return EDYNHIP_ERR_INVALID;
    if (flags & ~(uint32_t)EDYNHIP_RAYCAST_BRUTE_FORCE) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_raycast_device: unknown flag bits");
    if (n == 0) return EDYNHIP_OK;
    EH_TRY(query_begin(w));
    for (uint32_t off = 0; off < n; off += kWorldChunk)
        EH_TRY(world_raycast_chunk(w, std::min(kWorldChunk, n - off), (const float4 *)p0_f4 + off, (const float4 *)p1_f4 + off, num_ignore, ignore, flags,
                                   (edynhip_raycast_hit *)out + off));
    return EDYNHIP_OK;
}

int edynhip_world_raycast(edynhip_world *w, uint32_t n, const float *p0, const float *p1, uint32_t num_ignore, const uint32_t *ignore, uint32_t flags,
                          edynhip_raycast_hit *out) {
    if (!w || (n && (!p0 || !p1 || !out)) || (num_ignore && !ignore)) return EDYNHIP_ERR_INVALID;
    if (flags & ~(uint32_t)EDYNHIP_RAYCAST_BRUTE_FORCE) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_raycast: unknown flag bits");
    if (n == 0) return EDYNHIP_OK;
    EH_TRY(query_begin(w));
    const uint32_t chunk = std::min(n, kWorldChunk);
    W_HIP(w, w->h_in.grow(2 * (size_t)chunk * sizeof(float4)));
    W_HIP(w, w->h_out.grow((size_t)chunk * sizeof(edynhip_raycast_hit)));
    w->q_stage.resize(2 * (size_t)chunk);
    for (uint32_t off = 0; off < n; off += kWorldChunk) {
        const uint32_t m = std::min(kWorldChunk, n - off);
        for (uint32_t r = 0; r < m; ++r) {
            const float *q0 = p0 + 3 * ((size_t)off + r), *q1 = p1 + 3 * ((size_t)off + r);
            w->q_stage[r] = make_float4(q0[0], q0[1], q0[2], 0.0f);
            w->q_stage[(size_t)chunk + r] = make_float4(q1[0], q1[1], q1[2], 0.0f);
        }
        W_HIP(w, hipSetDevice(w->devices[0]));
        float4 *d = (float4 *)w->h_in.h;
        W_HIP(w, hipMemcpyAsync(d, w->q_stage.data(), (size_t)m * sizeof(float4), hipMemcpyHostToDevice, w->qstream));
        W_HIP(w, hipMemcpyAsync(d + chunk, w->q_stage.data() + chunk, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, w->qstream));
        W_HIP(w, hipStreamSynchronize(w->qstream));
        EH_TRY(world_raycast_chunk(w, m, d, d + chunk, num_ignore, ignore, flags, w->h_out.h));
        W_HIP(w, hipMemcpyAsync(out + off, w->h_out.h, (size_t)m * sizeof(edynhip_raycast_hit), hipMemcpyDeviceToHost, w->qstream));
        W_HIP(w, hipStreamSynchronize(w->qstream));
    }
    return EDYNHIP_OK;
}

int edynhip_world_query_aabb_device(edynhip_world *w, int category, uint32_t n, const void *boxes_f4, uint32_t flags, void *offsets, void *ids,
                                    uint32_t capacity, void *total) {
    if (!w || !offsets || !total || (n && !boxes_f4)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_world_query(w, category, flags, "edynhip_world_query_aabb_device"));
    EH_TRY(query_begin(w));
    unsigned long long tot = 0;
    EH_TRY(world_query_count(w, category, n, (const float4 *)boxes_f4, flags, (uint32_t *)offsets, (uint32_t *)total, &tot));
    if (!ids || capacity == 0 || tot == 0) return EDYNHIP_OK;
    return world_query_fill(w, category, n, flags, (const uint32_t *)offsets, (uint32_t *)ids, capacity);
}

int edynhip_world_query_aabb(edynhip_world *w, int category, uint32_t n, const float *boxes6, uint32_t flags, uint32_t *offsets, uint32_t *ids,
                             uint32_t capacity, uint32_t *total) {
    if (!w || !offsets || !total || (n && !boxes6)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_world_query(w, category, flags, "edynhip_world_query_aabb"));
    EH_TRY(query_begin(w));
    W_HIP(w, w->h_in.grow(std::max<size_t>(2 * (size_t)n, 1) * sizeof(float4)));
    W_HIP(w, w->h_off_out.grow(((size_t)n + 2) * sizeof(uint32_t)));
    w->q_stage.resize(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        const float *b = boxes6 + 6 * (size_t)i;
        w->q_stage[2 * (size_t)i] = make_float4(b[0], b[1], b[2], 0.0f);
        w->q_stage[2 * (size_t)i + 1] = make_float4(b[3], b[4], b[5], 0.0f);
    }
    if (n) W_HIP(w, hipMemcpyAsync(w->h_in.h, w->q_stage.data(), 2 * (size_t)n * sizeof(float4), hipMemcpyHostToDevice, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    uint32_t *d_off = (uint32_t *)w->h_off_out.h;
    unsigned long long tot = 0;
    EH_TRY(world_query_count(w, category, n, (const float4 *)w->h_in.h, flags, d_off, d_off + n + 1, &tot));
    W_HIP(w, hipMemcpyAsync(offsets, d_off, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    *total = tot >= kSat32 ? 0xFFFFFFFFu : (uint32_t)tot;
    if (!ids) return EDYNHIP_OK;
    if (tot > capacity || tot >= kSat32) return w->fail(EDYNHIP_ERR_CAPACITY, "edynhip_world_query_aabb: capacity (offsets and total are valid: size ids by *total and ask again)");
    if (tot == 0) return EDYNHIP_OK;
    W_HIP(w, w->h_ids_out.grow((size_t)tot * sizeof(uint32_t)));
    EH_TRY(world_query_fill(w, category, n, flags, d_off, (uint32_t *)w->h_ids_out.h, (uint32_t)tot));
    W_HIP(w, hipMemcpyAsync(ids, w->h_ids_out.h, (size_t)tot * sizeof(uint32_t), hipMemcpyDeviceToHost, w->qstream));
    W_HIP(w, hipStreamSynchronize(w->qstream));
    return EDYNHIP_OK;
}

}  // extern "C"
