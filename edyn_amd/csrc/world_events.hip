// Contact events and point ids on a multi-device world (multi.hip edynhip_world_get_contact_events / edynhip_world_get_point_ids): what a
// shard context does for the world beside its own step. A shard records its events natively in world terms - EventSink::step counts the
// world's steps (edynhip_ctx::event_step_base) and the narrowphase tags every id it issues with the shard (event_id_tag) - so what is left:
//   - after every step, the step's event records with their LOCAL body indices mapped to global ones (k_world_translate_events), into a
//     block of the shard's own that the world appends to its list on the home device;
//   - the slot-major id columns of the current manifold array as one [m][4] table in edynhip_get_manifolds order (k_world_gather_pids),
//     and back (k_world_inject_pids): the ids of carried points, put in place after edynhip_set_manifolds has re-issued them.
// All three stream: one record / one manifold per lane, no LDS, no atomics.
#include "ctx.hpp"

namespace eh {

// One event per lane: 24 bytes in (16 + 8), 24 bytes out. The count is the device counter's (the list may have overflowed: `cap` bounds it).
__global__ void __launch_bounds__(256) k_world_translate_events(const ContactEvent *__restrict__ in, const uint32_t *__restrict__ count, uint32_t cap,
                                                                const uint32_t *__restrict__ local_ids, uint32_t n_local, ContactEvent *__restrict__ out) {
    const uint32_t held = min(*count, cap);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < held; i += gridDim.x * blockDim.x) {
        const uint4 head = *(const uint4 *)__builtin_assume_aligned(&in[i], 8);   // type, step, bodyA, bodyB
        const uint64_t pid = in[i].pid;
        uint4 o = head;
        if (head.z < n_local) o.z = local_ids[head.z];
        if (head.w < n_local) o.w = local_ids[head.w];
        ContactEvent e;
        e.type = o.x; e.step = o.y; e.bodyA = o.z; e.bodyB = o.w; e.pid = pid;
        out[i] = e;
    }
}

// The tail [first, last) of the list, what an edit appended behind the last step's events (edynhip_world_edit_bodies): the host has read
// both counts, out[i - first] takes record i. One event per lane as above.
__global__ void __launch_bounds__(256) k_world_translate_event_tail(const ContactEvent *__restrict__ in, uint32_t first, uint32_t last,
                                                                    const uint32_t *__restrict__ local_ids, uint32_t n_local, ContactEvent *__restrict__ out) {
    const uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= last) return;
    const uint4 head = *(const uint4 *)__builtin_assume_aligned(&in[i], 8);   // type, step, bodyA, bodyB
    ContactEvent e;
    e.type = head.x; e.step = head.y;
    e.bodyA = head.z < n_local ? local_ids[head.z] : head.z;
    e.bodyB = head.w < n_local ? local_ids[head.w] : head.w;
    e.pid = in[i].pid;
    out[i - first] = e;
}

// ids[4 m + k] = id of point k of manifold m, 0 where there is no point
__global__ void __launch_bounds__(256) k_world_gather_pids(uint32_t M, const uint64_t *__restrict__ pid, uint32_t cap, const uint32_t *__restrict__ info,
                                                           uint64_t *__restrict__ ids) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t np = info[m] & 0xFFu;
    uint64_t v[kMaxPts];
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k) v[k] = k < np ? pid[slot_at(cap, k, m)] : 0ull;
    ulonglong2 *o = (ulonglong2 *)(ids + 4 * (size_t)m);   // (32 bytes per manifold: 16-byte aligned)
    o[0] = make_ulonglong2(v[0], v[1]);
    o[1] = make_ulonglong2(v[2], v[3]);
}

__global__ void __launch_bounds__(256) k_world_inject_pids(uint32_t M, const uint64_t *__restrict__ ids, uint64_t *__restrict__ pid, uint32_t cap,
                                                           const uint32_t *__restrict__ info) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t np = info[m] & 0xFFu;
    const ulonglong2 *s = (const ulonglong2 *)(ids + 4 * (size_t)m);
    const ulonglong2 a = s[0], b = s[1];
    const uint64_t v[kMaxPts] = {a.x, a.y, b.x, b.y};
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPts; ++k) if (k < np) pid[slot_at(cap, k, m)] = v[k];
}

int shard_translate_events(edynhip_ctx *c, uint32_t expected, const uint32_t *local_ids_dev, uint32_t n_local, void *out) {
    if (!c->events) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "shard_translate_events: the context records no events");
    const uint32_t n = std::min(expected, c->event_cap);
    if (n == 0) return EDYNHIP_OK;
    hipLaunchKernelGGL(k_world_translate_events, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const ContactEvent *)c->events, (const uint32_t *)c->event_count,
                       c->event_cap, local_ids_dev, n_local, (ContactEvent *)out);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

int shard_translate_event_tail(edynhip_ctx *c, uint32_t first, uint32_t last, const uint32_t *local_ids_dev, uint32_t n_local, void *out) {
    if (!c->events) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "shard_translate_event_tail: the context records no events");
    last = std::min(last, c->event_cap);   // (out holds event_cap records: last - first of them are written)
    if (first >= last) return EDYNHIP_OK;
    hipLaunchKernelGGL(k_world_translate_event_tail, dim3((last - first + 255) / 256), dim3(256), 0, c->stream, (const ContactEvent *)c->events, first, last,
                       local_ids_dev, n_local, (ContactEvent *)out);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

int shard_gather_point_ids(edynhip_ctx *c, uint64_t *ids_dev) {
    const Manifolds &mf = c->m[c->cur];
    if (!mf.pid) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "shard_gather_point_ids: the context records no events");
    const uint32_t M = c->num_manifolds;
    if (M == 0) return EDYNHIP_OK;
    hipLaunchKernelGGL(k_world_gather_pids, dim3((M + 255) / 256), dim3(256), 0, c->stream, M, (const uint64_t *)mf.pid, mf.cap, (const uint32_t *)mf.info, ids_dev);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

int shard_inject_point_ids(edynhip_ctx *c, const uint64_t *ids_dev, uint32_t M) {
    const Manifolds &mf = c->m[c->cur];
    if (!mf.pid) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "shard_inject_point_ids: the context records no events");
    if (M != c->num_manifolds) return set_error(c, EDYNHIP_ERR_INVALID, "shard_inject_point_ids: one row per manifold of the current array");
    if (M == 0) return EDYNHIP_OK;
    hipLaunchKernelGGL(k_world_inject_pids, dim3((M + 255) / 256), dim3(256), 0, c->stream, M, ids_dev, mf.pid, mf.cap, (const uint32_t *)mf.info);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

}  // namespace eh
