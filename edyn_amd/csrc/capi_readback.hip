// C-ABI, read-back (include/edynhip.h): get / set of the packed state, derived state and sleep flags, the manifold record round
// trip, contact events and point ids, and the three generations of asynchronous read-back - edynhip_snapshot, the record
// snapshots and the contact-event prefetch - with the side stream they share.
#include "ctx.hpp"
#include "ctx_rules.hpp"
#include "dstep.hpp"
#include "drecord.hpp"
#include <algorithm>
#include <cstring>

namespace eh {
using namespace dm;

__global__ void k_manifolds_to_records(uint32_t M, Manifolds mf, edynhip_manifold *out) {
    uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    edynhip_manifold r;
    memset(&r, 0, sizeof(r));
    r.body[0] = mf.bodyA[m]; r.body[1] = mf.bodyB[m];
    const uint32_t info = mf.info[m];
    r.num_points = info & 0xFF; r.colour = info >> 8;
    for (uint32_t k = 0; k < r.num_points; ++k) {
        const size_t s = pt_at(mf.cap, k, m);
        float4 a = mf.pA[s], b = mf.pB[s], n = mf.nrm[s], l = mf.lnrm[s], im = mf.imp[s];
        edynhip_point &p = r.pt[k];
        p.pivotA[0] = a.x; p.pivotA[1] = a.y; p.pivotA[2] = a.z; p.distance = a.w;
        p.pivotB[0] = b.x; p.pivotB[1] = b.y; p.pivotB[2] = b.z; p.friction = b.w;
        p.normal[0] = n.x; p.normal[1] = n.y; p.normal[2] = n.z; p.attachment = __float_as_int(n.w);
        p.local_normal[0] = l.x; p.local_normal[1] = l.y; p.local_normal[2] = l.z; p.restitution = l.w;
        p.normal_impulse = im.x; p.friction_impulse[0] = im.y; p.friction_impulse[1] = im.z; p.lifetime = __float_as_uint(im.w);
    }
    out[m] = r;
}
__global__ void k_records_to_manifolds(uint32_t M, const edynhip_manifold *in, Manifolds mf, const uint32_t *__restrict__ flags,
                                       const float4 *__restrict__ mat2) {
    uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const edynhip_manifold r = in[m];
    const uint32_t a = r.body[0], b = r.body[1];
    auto owner_of = [&](const edynhip_manifold &x) { return pair_owner(x.body[0], x.body[1], (flags[x.body[0]] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC, (flags[x.body[1]] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC); };
    const uint32_t hi = owner_of(r), lo = hi == a ? b : a;
    mf.skey[m] = ((((uint64_t)hi << 32) | lo) << 1) | (a == lo ? 1u : 0u);
    mf.bodyA[m] = a; mf.bodyB[m] = b;
    {
        const uint32_t ph = m > 0 ? owner_of(in[m - 1]) : 0xFFFFFFFFu;
        const uint32_t nh = m + 1 < M ? owner_of(in[m + 1]) : 0xFFFFFFFFu;
        if (ph != hi) mf.seg_start[hi] = m;
        if (nh != hi) mf.seg_end[hi] = m + 1;
    }
    mf.info[m] = (r.num_points & 0xFF) | ((r.colour & 0xFF) << 8);
    mf.tree[m] = 0;   // (set_manifolds forces a full island update, which rebuilds the certificate)
    for (uint32_t k = 0; k < r.num_points; ++k) {
        const size_t t = pt_at(mf.cap, k, m), s = slot_at(mf.cap, k, m);
        const edynhip_point &p = r.pt[k];
        mf.pA[t] = make_float4(p.pivotA[0], p.pivotA[1], p.pivotA[2], p.distance);
        mf.pB[t] = make_float4(p.pivotB[0], p.pivotB[1], p.pivotB[2], p.friction);
        mf.nrm[t] = make_float4(p.normal[0], p.normal[1], p.normal[2], __int_as_float(p.attachment));
        mf.lnrm[t] = make_float4(p.local_normal[0], p.local_normal[1], p.local_normal[2], p.restitution);
        mf.imp[t] = make_float4(p.normal_impulse, p.friction_impulse[0], p.friction_impulse[1], __uint_as_float(p.lifetime));
        if (mf.pid) mf.pid[s] = ((uint64_t)m << 2) | k;   // injected points: high word 0
        if (mf.xmat) {   // the record carries no extras: the materials are mixed as for a new point, the extras impulses start at 0
            const float4 ma = mat2[a], mb = mat2[b];
            float stiff = kLarge, damp = kLarge;
            if (ma.z < kLarge || mb.z < kLarge) { stiff = 1.0f / (1.0f / ma.z + 1.0f / mb.z); damp = 1.0f / (1.0f / ma.w + 1.0f / mb.w); }
            mf.xmat[s] = make_float4(fmaxf(ma.y, mb.y), fmaxf(ma.x, mb.x), stiff, damp);
            mf.ximp[s] = make_float4(0, 0, 0, 0);
        }
    }
}
__global__ void k_pack_state(uint32_t first, uint32_t count, Bodies b, float *dst) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const uint32_t i = first + t;
    float4 p = B_POS(b, i), q = B_ORN(b, i), v = b.linvel[i], w = b.angvel[i];
    float *o = dst + (size_t)t * 13;
    o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w;
    o[7] = v.x; o[8] = v.y; o[9] = v.z; o[10] = w.x; o[11] = w.y; o[12] = w.z;
}
__global__ void k_unpack_state(uint32_t n, const float *src, Bodies b) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *o = src + (size_t)i * 13;
    B_POS(b, i) = make_float4(o[0], o[1], o[2], B_POS(b, i).w);
    B_ORN(b, i) = make_float4(o[3], o[4], o[5], o[6]);
    b.linvel[i] = make_float4(o[7], o[8], o[9], 0);
    b.angvel[i] = make_float4(o[10], o[11], o[12], 0);
}
__global__ void k_pack_derived(uint32_t n, Bodies b, float *aabb, float *iw) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 a = b.amin[i], c = b.amax[i];
    aabb[6 * i] = a.x; aabb[6 * i + 1] = a.y; aabb[6 * i + 2] = a.z; aabb[6 * i + 3] = c.x; aabb[6 * i + 4] = c.y; aabb[6 * i + 5] = c.z;
    for (int r = 0; r < 3; ++r) { float4 x = B_IW(b, i, r); iw[9 * i + 3 * r] = x.x; iw[9 * i + 3 * r + 1] = x.y; iw[9 * i + 3 * r + 2] = x.z; }
}

// The stream the read-back copies run on and the event that puts it behind the stepper's: made by whichever read-back comes first
static int ensure_side_stream(edynhip_ctx *c) {
    if (c->side.stream) return EDYNHIP_OK;
    EH_HIP(c, c->side.stream.create(hipStreamNonBlocking));
    EH_HIP(c, c->side.ready.create(hipEventDisableTiming));
    return EDYNHIP_OK;
}

// The call's event count and list go to the pinned prefetch buffer on the side stream, behind what c->stream has enqueued so far
int enqueue_event_prefetch(edynhip_ctx *c) {
    EventPrefetch &p = c->evp;
    EH_HIP(c, hipEventRecord(p.np_done, c->stream));
    EH_HIP(c, hipStreamWaitEvent(c->side.stream, p.np_done, 0));
    EH_HIP(c, hipMemcpyAsync(p.host, c->event_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->side.stream));
    EH_HIP(c, hipMemcpyAsync(p.host + 64, c->events, (size_t)std::min(p.max, c->event_cap) * sizeof(eh::ContactEvent), hipMemcpyDeviceToHost, c->side.stream));
    EH_HIP(c, hipEventRecord(p.ready, c->side.stream));
    p.state = 1;
    return EDYNHIP_OK;
}

}  // namespace eh

using namespace eh;

extern "C" {

int edynhip_get_state(edynhip_ctx *c, float *pos, float *orn, float *linvel, float *angvel) {
    if (!c) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    float *d = c->state.dev;
    const float *h = c->state.host;
    hipLaunchKernelGGL(k_pack_state, dim3(blocks(n, 256)), dim3(256), 0, c->stream, 0u, n, c->b, d);
    hipError_t e = hipMemcpyAsync(c->state.host, d, (size_t)n * 13 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_get_state", e);
    for (uint32_t i = 0; i < n; ++i) {
        const float *o = &h[(size_t)i * 13];
        if (pos) std::memcpy(pos + 3 * i, o, 12);
        if (orn) std::memcpy(orn + 4 * i, o + 3, 16);
        if (linvel) std::memcpy(linvel + 3 * i, o + 7, 12);
        if (angvel) std::memcpy(angvel + 3 * i, o + 10, 12);
    }
    return EDYNHIP_OK;
}

int edynhip_set_state(edynhip_ctx *c, const float *pos, const float *orn, const float *linvel, const float *angvel) {
    if (!c || !pos || !orn || !linvel || !angvel) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(flush_joint_redefs(c));   // pending angle resets refer to the orientations before this edit
    float *h = c->state.host, *d = c->state.dev;
    for (uint32_t i = 0; i < n; ++i) {
        float *o = &h[(size_t)i * 13];
        std::memcpy(o, pos + 3 * i, 12); std::memcpy(o + 3, orn + 4 * i, 16);
        std::memcpy(o + 7, linvel + 3 * i, 12); std::memcpy(o + 10, angvel + 3 * i, 12);
    }
    hipError_t e = hipMemcpyAsync(d, h, (size_t)n * 13 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_unpack_state, dim3(blocks(n, 256)), dim3(256), 0, c->stream, n, d, c->b);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the staging buffers are reused by the next call
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_set_state", e);
    invalidate_bodies_moved(c);   // moved behind the broadphase's back: the candidate lists are rebuilt at the next step
    // (The AABBs stay those of the old state until the end of the next step. edynhip_world_set_state in multi_edit.hip relies on it: it runs
    // its approach check AFTER that step, when the boxes - and the first new pairs - can first exist. Refreshing the boxes here would
    // need the check before the step there.)
    if (c->sleeping) return edynhip_wake_all(c);   // an edited body wakes its island (wake_up_entity); all of them here
    return EDYNHIP_OK;
}

int edynhip_refresh_derived(edynhip_ctx *c) {
    if (!c) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    invalidate_bodies_moved(c);
    return refresh_derived(c);
}

int edynhip_get_asleep(edynhip_ctx *c, uint8_t *asleep) {
    if (!c || !asleep) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    std::vector<uint32_t> fl(n);
    EH_HIP(c, hipMemcpyAsync(fl.data(), c->b.flags, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i) asleep[i] = (fl[i] & BF_ASLEEP) ? 1 : 0;
    return EDYNHIP_OK;
}

int edynhip_pack_state_device(edynhip_ctx *c, void *dst, uint32_t first, uint32_t count) {
    if (!c || !dst || (uint64_t)first + count > c->b.n) return EDYNHIP_ERR_INVALID;
    if (count == 0) return EDYNHIP_OK;
    hipLaunchKernelGGL(k_pack_state, dim3(blocks(count, 256)), dim3(256), 0, c->stream, first, count, c->b, (float *)dst);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

int edynhip_get_derived(edynhip_ctx *c, float *aabb, float *iw, uint32_t *island) {
    if (!c) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    DeviceBuf<float> d;
    EH_HIP(c, d.alloc((size_t)n * 15));
    hipLaunchKernelGGL(k_pack_derived, dim3(blocks(n, 256)), dim3(256), 0, c->stream, n, c->b, (float *)d, d + (size_t)n * 6);
    hipError_t e = hipSuccess;
    if (aabb) e = hipMemcpyAsync(aabb, d, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && iw) e = hipMemcpyAsync(iw, d + (size_t)n * 6, (size_t)n * 9 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && island) e = hipMemcpyAsync(island, c->b.island, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_get_derived", e);
    return EDYNHIP_OK;
}

int edynhip_num_manifolds(edynhip_ctx *c, uint32_t *n) {
    if (!c || !n) return EDYNHIP_ERR_INVALID;
    *n = c->num_manifolds;
    return EDYNHIP_OK;
}

int edynhip_get_manifolds(edynhip_ctx *c, edynhip_manifold *out, uint32_t capacity, uint32_t *n) {
    if (!c || !n) return EDYNHIP_ERR_INVALID;
    const uint32_t M = c->num_manifolds;
    *n = M;
    if (M == 0 || !out) return EDYNHIP_OK;
    if (capacity < M) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_manifolds: capacity too small");
    EH_HIP(c, hipSetDevice(c->device));
    DeviceBuf<edynhip_manifold> d;
    EH_HIP(c, d.alloc(M));
    hipLaunchKernelGGL(k_manifolds_to_records, dim3(blocks(M, 128)), dim3(128), 0, c->stream, M, c->m[c->cur], (edynhip_manifold *)d);
    hipError_t e = hipMemcpyAsync(out, d, (size_t)M * sizeof(edynhip_manifold), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_get_manifolds", e);
    return EDYNHIP_OK;
}

int edynhip_set_manifolds(edynhip_ctx *c, const edynhip_manifold *in, uint32_t n) {
    if (!c || (n && !in)) return EDYNHIP_ERR_INVALID;
    if (n > c->m[c->cur].cap) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_set_manifolds: n > max_manifolds");
    EH_HIP(c, hipSetDevice(c->device));
    for (uint32_t i = 0; i < n; ++i)
        if (in[i].body[0] >= c->b.n || in[i].body[1] >= c->b.n || in[i].num_points > (uint32_t)kMaxPts)
            return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_manifolds: body index or point count out of range");
    // records must arrive in ascending canonical key order (the order edynhip_get_manifolds returns)
    auto key = [&](uint32_t i) -> uint64_t {
        const uint32_t a = in[i].body[0], b = in[i].body[1];
        if (a >= c->b.n || b >= c->b.n) return (uint64_t)~0ull;
        return canonical_pair_key(a, b, c->host_kind[a] == EDYNHIP_KIND_DYNAMIC, c->host_kind[b] == EDYNHIP_KIND_DYNAMIC);
    };
    if (!strictly_ascending(n, key)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_manifolds: records not sorted by canonical pair key");
    c->num_manifolds = n;
    invalidate_contact_state_replaced(c);
    // colouring state that travels with the records: the number of colours in use (the next step releases the top one)
    c->num_colours = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (in[i].colour != kNoColour && in[i].num_points > 0 && in[i].colour + 1 > c->num_colours) c->num_colours = in[i].colour + 1;
    EH_HIP(c, hipMemsetAsync(c->m[c->cur].seg_start, 0, (size_t)c->b.cap * sizeof(uint32_t), c->stream));
    EH_HIP(c, hipMemsetAsync(c->m[c->cur].seg_end, 0, (size_t)c->b.cap * sizeof(uint32_t), c->stream));
    if (n == 0) return EDYNHIP_OK;
    DeviceBuf<edynhip_manifold> d;
    EH_HIP(c, d.alloc(n));
    hipError_t e = hipMemcpyAsync(d, in, (size_t)n * sizeof(edynhip_manifold), hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_records_to_manifolds, dim3(blocks(n, 128)), dim3(128), 0, c->stream, n, (const edynhip_manifold *)d, c->m[c->cur], c->b.flags, c->b.mat2);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_set_manifolds", e);
    return EDYNHIP_OK;
}

int edynhip_get_point_extras(edynhip_ctx *c, float *out7, uint32_t capacity, uint32_t *n) {
    if (!c || !n) return EDYNHIP_ERR_INVALID;
    if (c->world_shard) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "edynhip_get_point_extras: a shard of a multi-device world is read through edynhip_world_get_point_extras");
    const uint32_t M = c->num_manifolds;
    *n = M;
    if (M == 0 || !out7) return EDYNHIP_OK;
    if (capacity < M) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_point_extras: capacity too small");
    EH_HIP(c, hipSetDevice(c->device));
    const Manifolds &mf = c->m[c->cur];
    std::vector<uint32_t> info(M);
    EH_HIP(c, hipMemcpyAsync(info.data(), mf.info, (size_t)M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<float4> xm(M), xi(M);
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k) {
        if (mf.xmat) {
            EH_HIP(c, hipMemcpyAsync(xm.data(), mf.xmat + (size_t)k * mf.cap, (size_t)M * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
            EH_HIP(c, hipMemcpyAsync(xi.data(), mf.ximp + (size_t)k * mf.cap, (size_t)M * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
            EH_HIP(c, hipStreamSynchronize(c->stream));
        }
        for (uint32_t m = 0; m < M; ++m) {
            float *o = out7 + ((size_t)4 * m + k) * 7;
            const bool live = k < (info[m] & 0xFF);
            const float4 a = mf.xmat ? xm[m] : make_float4(0, 0, kLarge, kLarge), b = mf.xmat ? xi[m] : make_float4(0, 0, 0, 0);
            o[0] = live ? b.x : 0; o[1] = live ? b.y : 0; o[2] = live ? b.z : 0;
            o[3] = live ? a.x : 0; o[4] = live ? a.y : 0; o[5] = live ? a.z : 0; o[6] = live ? a.w : 0;
        }
    }
    return EDYNHIP_OK;
}

int edynhip_get_contact_events(edynhip_ctx *c, edynhip_contact_event *out, uint32_t capacity, uint32_t *n) {
    static_assert(sizeof(edynhip_contact_event) == sizeof(ContactEvent), "event record layout");
    if (!c || !n) return EDYNHIP_ERR_INVALID;
    *n = 0;
    if (!c->events) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "edynhip_get_contact_events: create the context with EDYNHIP_FLAG_CONTACT_EVENTS");
    EH_HIP(c, hipSetDevice(c->device));
    uint32_t count = 0;
    EH_HIP(c, hipMemcpyAsync(&count, c->event_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    const uint32_t held = std::min(count, c->event_cap);
    *n = held;
    if (out) {
        if (capacity < held) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_contact_events: capacity too small");
        if (held) {
            EH_HIP(c, hipMemcpyAsync(out, c->events, (size_t)held * sizeof(ContactEvent), hipMemcpyDeviceToHost, c->stream));
            EH_HIP(c, hipStreamSynchronize(c->stream));
        }
    }
    if (count > c->event_cap) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_contact_events: more events than the context holds; resynchronise from edynhip_get_manifolds");
    return EDYNHIP_OK;
}
int edynhip_get_point_ids(edynhip_ctx *c, uint64_t *ids, uint32_t capacity, uint32_t *n) {
    if (!c || !n) return EDYNHIP_ERR_INVALID;
    const uint32_t M = c->num_manifolds;
    *n = M;
    if (!c->events) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "edynhip_get_point_ids: create the context with EDYNHIP_FLAG_CONTACT_EVENTS");
    if (M == 0 || !ids) return EDYNHIP_OK;
    if (capacity < M) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_point_ids: capacity too small");
    EH_HIP(c, hipSetDevice(c->device));
    const Manifolds &mf = c->m[c->cur];
    std::vector<uint64_t> col(M);
    std::vector<uint32_t> info(M);
    EH_HIP(c, hipMemcpyAsync(info.data(), mf.info, (size_t)M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k) {
        EH_HIP(c, hipMemcpyAsync(col.data(), mf.pid + (size_t)k * mf.cap, (size_t)M * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        EH_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t m = 0; m < M; ++m) ids[(size_t)4 * m + k] = k < (info[m] & 0xFF) ? col[m] : 0;
    }
    return EDYNHIP_OK;
}

int edynhip_get_pairs(edynhip_ctx *c, uint64_t *keys, uint32_t capacity, uint32_t *n) {
    if (!c || !n) return EDYNHIP_ERR_INVALID;
    const uint32_t M = c->num_manifolds;
    *n = M;
    if (M == 0 || !keys) return EDYNHIP_OK;
    if (capacity < M) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_get_pairs: capacity too small");
    EH_HIP(c, hipSetDevice(c->device));
    EH_HIP(c, hipMemcpyAsync(keys, c->m[c->cur].skey, (size_t)M * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < M; ++i) {   // drop the orientation bit; (owner, other) -> the documented (max, min)
        const uint32_t a = (uint32_t)(keys[i] >> 33), b = (uint32_t)(keys[i] >> 1);
        keys[i] = ((uint64_t)std::max(a, b) << 32) | std::min(a, b);
    }
    std::sort(keys, keys + M);
    return EDYNHIP_OK;
}

// ---- double-buffered read-back (simulation_worker.cpp:406-444: finished steps are handed over while the next one runs)
int edynhip_snapshot(edynhip_ctx *c) {
    if (!c) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    SnapshotSlots &sn = c->snap;
    const uint32_t n = c->b.n;
    const int slot = (sn.last + 1) & 1;
    EH_TRY(ensure_side_stream(c));
    if (!sn.dev[1]) {
        for (int k = 0; k < 2; ++k) {
            EH_HIP(c, sn.event[k].create(hipEventDisableTiming));
            EH_HIP(c, sn.host[k].alloc((size_t)c->b.cap * 13));
            EH_TRY(dalloc(c, sn.dev[k], (size_t)c->b.cap * 13));
        }
    }
    // pack on the stepper's stream (it must see the finished step), copy on the side stream: the copy engine moves the
    // bytes while the stepper's next kernels already run
    if (n) hipLaunchKernelGGL(k_pack_state, dim3(blocks(n, 256)), dim3(256), 0, c->stream, 0u, n, c->b, sn.dev[slot]);
    EH_HIP(c, hipEventRecord(c->side.ready, c->stream));
    EH_HIP(c, hipStreamWaitEvent(c->side.stream, c->side.ready, 0));
    if (n) EH_HIP(c, hipMemcpyAsync(sn.host[slot], sn.dev[slot], (size_t)n * 13 * sizeof(float), hipMemcpyDeviceToHost, c->side.stream));
    EH_HIP(c, hipEventRecord(sn.event[slot], c->side.stream));
    sn.step[slot] = c->step_index; sn.bodies[slot] = n; sn.last = slot;
    return EDYNHIP_OK;
}
int edynhip_snapshot_read(edynhip_ctx *c, float *pos, float *orn, float *linvel, float *angvel, uint32_t *step_index) {
    if (!c) return EDYNHIP_ERR_INVALID;
    if (c->snap.last < 0) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_snapshot_read: no snapshot was taken");
    EH_HIP(c, hipSetDevice(c->device));
    const int slot = c->snap.last;
    EH_HIP(c, hipEventSynchronize(c->snap.event[slot]));   // that copy only - not the steps enqueued after it
    const float *h = c->snap.host[slot];
    for (uint32_t i = 0; i < c->snap.bodies[slot]; ++i) {
        const float *o = &h[(size_t)i * 13];
        if (pos) std::memcpy(pos + 3 * i, o, 12);
        if (orn) std::memcpy(orn + 4 * i, o + 3, 16);
        if (linvel) std::memcpy(linvel + 3 * i, o + 7, 12);
        if (angvel) std::memcpy(angvel + 3 * i, o + 10, 12);
    }
    if (step_index) *step_index = c->snap.step[slot];
    return EDYNHIP_OK;
}

// ---- record snapshots: the registry write-back read in place (edynhip.h, ABI 15)
static_assert(sizeof(edynhip_body_record) == 96, "record layout");
constexpr size_t kRecHeader = 64;   // [0] = events that occurred, [1] = events copied into this block
__global__ void k_pack_records(uint32_t n, Bodies b, float present_dt, float4 *__restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 rec[6];
    body_record(b, i, present_dt, rec);   // drecord.hpp: shared with the multi-device world's pack
    float4 *o = dst + (size_t)i * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = rec[k];
}
__global__ void k_pack_events(const eh::ContactEvent *__restrict__ events, const uint32_t *__restrict__ count, uint32_t cap, uint32_t max_copy,
                              uint32_t *__restrict__ header, eh::ContactEvent *__restrict__ dst) {
    const uint32_t total = events ? *count : 0u;
    const uint32_t held = min(min(total, cap), max_copy);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { header[0] = total; header[1] = held; }
    for (uint32_t k = t; k < held; k += gridDim.x * blockDim.x) dst[k] = events[k];
}
int edynhip_snapshot_records(edynhip_ctx *c, float present_dt, uint32_t max_events, uint32_t flags) {
    if (!c) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    RecordSlots &rs = c->rec;
    const uint32_t n = c->b.n;
    const int slot = (rs.last + 1) & 1;
    EH_TRY(ensure_side_stream(c));
    if (!rs.dev[0]) {
        rs.event_cap = c->events ? std::min<uint32_t>(c->event_cap, std::max<uint32_t>(4096u, 2u * c->b.cap)) : 0u;
        const size_t bytes = kRecHeader + (size_t)rs.event_cap * sizeof(eh::ContactEvent) + (size_t)c->b.cap * sizeof(edynhip_body_record);
        for (int k = 0; k < 2; ++k) {
            EH_HIP(c, rs.event[k].create(hipEventDisableTiming));
            EH_HIP(c, rs.host[k].alloc(bytes));
            EH_TRY(dalloc(c, rs.dev[k], bytes));
        }
    }
    const uint32_t copy_events = std::min(max_events, rs.event_cap);
    const size_t ev_bytes = (size_t)rs.event_cap * sizeof(eh::ContactEvent);
    uint8_t *d = rs.dev[slot], *h = rs.host[slot];
    // EDYNHIP_SNAPSHOT_DIRECT: the pack kernels store straight into the pinned host slot (it is mapped into the device's address space) on the
    // stepper's stream - no copy engine, no second stream, no event between the two. A/B on one box ("Round 6"): edyn::update in
    // sequential mode 705 -> 727 steps/s; in asynchronous mode, where nobody waits for the snapshot, the copy engine's overlap is worth as much
    // (785 / 759 against 764 / 765): the shim asks for it in its synchronous write-back only. (developer knob EDYNHIP_RECORDS_DIRECT=0 / 1 overrides)
    const long direct_env = c->knobs.records_direct;
    const bool direct = direct_env >= 0 ? direct_env != 0 : (flags & EDYNHIP_SNAPSHOT_DIRECT) != 0;
    c->paths |= direct ? EDYNHIP_PATH_RECORDS_DIRECT : EDYNHIP_PATH_RECORDS_COPY;
    if (direct) {
        if (n) hipLaunchKernelGGL(k_pack_records, dim3(blocks(n, 256)), dim3(256), 0, c->stream, n, c->b, present_dt, (float4 *)(h + kRecHeader + ev_bytes));
        hipLaunchKernelGGL(k_pack_events, dim3(copy_events > 4096 ? 64 : 4), dim3(256), 0, c->stream, (const eh::ContactEvent *)c->events, (const uint32_t *)c->event_count,
                           c->event_cap, copy_events, (uint32_t *)h, (eh::ContactEvent *)(h + kRecHeader));
        EH_HIP(c, hipEventRecord(rs.event[slot], c->stream));
        rs.step[slot] = c->step_index; rs.bodies[slot] = n; rs.events_copied[slot] = copy_events; rs.last = slot;
        return EDYNHIP_OK;
    }
    // pack on the stepper's stream (it must see the finished steps), copy on the side stream: the copy engine moves the bytes
    // while the stepper's next kernels already run
    if (n) hipLaunchKernelGGL(k_pack_records, dim3(blocks(n, 256)), dim3(256), 0, c->stream, n, c->b, present_dt, (float4 *)(d + kRecHeader + ev_bytes));
    hipLaunchKernelGGL(k_pack_events, dim3(copy_events > 4096 ? 64 : 4), dim3(256), 0, c->stream, (const eh::ContactEvent *)c->events, (const uint32_t *)c->event_count,
                       c->event_cap, copy_events, (uint32_t *)d, (eh::ContactEvent *)(d + kRecHeader));
    EH_HIP(c, hipEventRecord(c->side.ready, c->stream));
    EH_HIP(c, hipStreamWaitEvent(c->side.stream, c->side.ready, 0));
    EH_HIP(c, hipMemcpyAsync(h, d, kRecHeader + (size_t)copy_events * sizeof(eh::ContactEvent), hipMemcpyDeviceToHost, c->side.stream));
    if (n) EH_HIP(c, hipMemcpyAsync(h + kRecHeader + ev_bytes, d + kRecHeader + ev_bytes, (size_t)n * sizeof(edynhip_body_record), hipMemcpyDeviceToHost, c->side.stream));
    EH_HIP(c, hipEventRecord(rs.event[slot], c->side.stream));
    rs.step[slot] = c->step_index; rs.bodies[slot] = n; rs.events_copied[slot] = copy_events; rs.last = slot;
    return EDYNHIP_OK;
}
int edynhip_snapshot_map(edynhip_ctx *c, edynhip_record_view *view) {
    if (!c || !view) return EDYNHIP_ERR_INVALID;
    const RecordSlots &rs = c->rec;
    if (rs.last < 0) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_snapshot_map: no record snapshot was taken");
    EH_HIP(c, hipSetDevice(c->device));
    const int slot = rs.last;
    EH_HIP(c, hipEventSynchronize(rs.event[slot]));   // that copy only - not the steps enqueued after it
    const uint8_t *h = rs.host[slot];
    const uint32_t *header = (const uint32_t *)h;
    view->records = (const edynhip_body_record *)(h + kRecHeader + (size_t)rs.event_cap * sizeof(eh::ContactEvent));
    view->num_bodies = rs.bodies[slot];
    view->step_index = rs.step[slot];
    view->events = c->events ? (const edynhip_contact_event *)(h + kRecHeader) : nullptr;
    view->total_events = header[0];
    view->num_events = header[1];
    return EDYNHIP_OK;
}

// ---- contact-event prefetch: the events of a step call handed over while its solve still runs
int edynhip_set_event_prefetch(edynhip_ctx *c, uint32_t max_events) {
    if (!c) return EDYNHIP_ERR_INVALID;
    if (!c->events) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "edynhip_set_event_prefetch: create the context with EDYNHIP_FLAG_CONTACT_EVENTS");
    EH_HIP(c, hipSetDevice(c->device));
    EventPrefetch &p = c->evp;
    EH_HIP(c, hipStreamSynchronize(c->stream));
    if (c->side.stream) EH_HIP(c, hipStreamSynchronize(c->side.stream));
    p.host.reset();
    p.max = std::min(max_events, c->event_cap); p.state = 0;
    if (p.max == 0) return EDYNHIP_OK;
    EH_TRY(ensure_side_stream(c));
    if (!p.np_done) { EH_HIP(c, p.np_done.create(hipEventDisableTiming)); EH_HIP(c, p.ready.create(hipEventDisableTiming)); }
    EH_HIP(c, p.host.alloc(64 + (size_t)p.max * sizeof(eh::ContactEvent)));
    std::memset(p.host, 0, 64);
    return EDYNHIP_OK;
}
int edynhip_prefetched_events(edynhip_ctx *c, const edynhip_contact_event **events, uint32_t *num_events, uint32_t *total_events) {
    if (!c || !events || !num_events || !total_events) return EDYNHIP_ERR_INVALID;
    *events = nullptr; *num_events = 0; *total_events = 0;
    const EventPrefetch &p = c->evp;
    if (p.max == 0 || p.state == 0) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_prefetched_events: no step call ran with the prefetch enabled");
    if (p.state == 2) return EDYNHIP_OK;   // every island asleep: the call ran no step, nothing happened
    EH_HIP(c, hipSetDevice(c->device));
    EH_HIP(c, hipEventSynchronize(p.ready));   // that copy only: the step's solve may still be running
    const uint32_t total = *(const uint32_t *)(const uint8_t *)p.host;
    *total_events = total;
    *num_events = std::min(std::min(total, c->event_cap), p.max);
    *events = (const edynhip_contact_event *)(p.host + 64);
    return EDYNHIP_OK;
}

}  // extern "C"
