// Record hand-over of the multi-device world (multi.hpp).
//
// edynhip_snapshot_records / edynhip_snapshot_map on a multi-device world: every shard packs the records of the bodies it reports with the
// single context's arithmetic and stores them at their global indices straight into one of the world's two pinned slots
// (world_records.hip); the event block is one copy from the list on the home device, behind the shards' appends. A step call returns with
// every shard idle, so "behind the steps issued so far" holds by construction; the map waits for the snapshot's own events only.
#include "multi.hpp"

using namespace eh;
using namespace eh::world;

namespace {

// what is still being written into slot k (by the snapshot that used it last) has landed
int rec_wait(edynhip_world *w, int k) {
    for (Shard &s : w->shards) {
        if (!s.res.rec_pending[k]) continue;
        W_HIP(w, hipSetDevice(s.device));
        W_HIP(w, hipEventSynchronize(s.res.rec_ev[k]));
        s.res.rec_pending[k] = false;
    }
    if (w->rec[k].ev_pending) {
        W_HIP(w, hipSetDevice(w->devices[0]));
        W_HIP(w, hipEventSynchronize(w->rec_ev_done[k]));
        w->rec[k].ev_pending = false;
    }
    return EDYNHIP_OK;
}

// The record of a body that no context holds, from the world's own arrays and the scene description. By build_shard's rule every body
// is held by its owner or, replicated, by shard 0, so today this writes nothing; it keeps the slot complete should a partition ever leave
// a body out. Such a body is simulated by nobody: the state is the gathered one; the presentation follows dm::integrate's formula.
void host_record(const edynhip_world *w, uint32_t g, float dt, edynhip_body_record &o) {
    const HostScene &sc = w->scene;
    const float *p = &w->pos[3 * (size_t)g], *q = &w->orn[4 * (size_t)g], *v = &w->linvel[3 * (size_t)g], *a = &w->angvel[3 * (size_t)g];
    std::memcpy(o.pos, p, 12); std::memcpy(o.orn, q, 16); std::memcpy(o.linvel, v, 12); std::memcpy(o.angvel, a, 12);
    for (int d = 0; d < 3; ++d) o.present_pos[d] = p[d] + v[d] * dt;
    const float ws = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float t = ws < 0.001f ? 0.5f * dt - dt * dt * dt * (1.0f / 48.0f) * ws * ws : (float)std::sin((double)(0.5f * ws * dt)) / ws;
    const float r[4] = {a[0] * t, a[1] * t, a[2] * t, (float)std::cos((double)(0.5f * ws * dt))};
    float m[4] = {r[3] * q[0] + r[0] * q[3] + r[1] * q[2] - r[2] * q[1], r[3] * q[1] + r[1] * q[3] + r[2] * q[0] - r[0] * q[2],
                  r[3] * q[2] + r[2] * q[3] + r[0] * q[1] - r[1] * q[0], r[3] * q[3] - r[0] * q[0] - r[1] * q[1] - r[2] * q[2]};
    const float len = std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3]);
    for (int d = 0; d < 4; ++d) o.present_orn[d] = m[d] / len;
    const float *c = sc.com.empty() ? nullptr : &sc.com[3 * (size_t)g];
    const bool has_origin = c && !(c[0] == 0 && c[1] == 0 && c[2] == 0);
    std::memcpy(o.origin, p, 12);
    if (has_origin) {   // origin = pos + rotate(orn, -com)
        const float x[3] = {-c[0], -c[1], -c[2]}, u[3] = {2.0f * q[0], 2.0f * q[1], 2.0f * q[2]};
        const float k[3] = {q[1] * x[2] - q[2] * x[1] + q[3] * x[0], q[2] * x[0] - q[0] * x[2] + q[3] * x[1], q[0] * x[1] - q[1] * x[0] + q[3] * x[2]};
        o.origin[0] = p[0] + (x[0] + (u[1] * k[2] - u[2] * k[1])); o.origin[1] = p[1] + (x[1] + (u[2] * k[0] - u[0] * k[2])); o.origin[2] = p[2] + (x[2] + (u[0] * k[1] - u[1] * k[0]));
    }
    o.flags = (sc.kind[g] == EDYNHIP_KIND_DYNAMIC && !w->is_removed(g) ? EDYNHIP_RECORD_DYNAMIC : 0u) | (has_origin ? EDYNHIP_RECORD_HAS_ORIGIN : 0u) |
              (w->is_removed(g) ? EDYNHIP_RECORD_REMOVED : 0u);
}

}  // namespace

extern "C" {

int edynhip_world_snapshot_records(edynhip_world *w, float present_dt, uint32_t max_events, uint32_t flags) {
    static_assert(sizeof(edynhip_body_record) == 96 && sizeof(ContactEvent) == 24, "slot layout");
    if (!w) return EDYNHIP_ERR_INVALID;
    if (flags & ~(uint32_t)EDYNHIP_SNAPSHOT_DIRECT) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_snapshot_records: flags must be 0 or EDYNHIP_SNAPSHOT_DIRECT");
    EH_TRY(ensure_built(w));
    const int k = (w->rec_last + 1) & 1, home = w->devices[0];
    edynhip_world::RecSlot &sl = w->rec[k];
    EH_TRY(rec_wait(w, k));   // (a snapshot that was never mapped may still be writing into this slot)
    const uint32_t n = w->scene.n;
    const uint32_t copy = w->events_on() ? std::min(max_events, w->ev_n) : 0u;
    if (!sl.host || n > sl.body_cap || copy > sl.ev_cap) {
        // the views into this slot expired with this call (valid until the next-but-one): it may move. Portable and mapped: every shard's
        // device stores into it.
        // (sized for the scene as it stands; a slot that has to grow - bodies were added to the running world - takes head-room)
        const uint32_t body_cap = n <= sl.body_cap ? sl.body_cap : sl.body_cap ? n + n / 4 + 64 : n;
        const uint32_t ev_cap = w->events_on() ? std::max(std::max<uint32_t>(copy, 4096u), sl.ev_cap) : 0u;
        W_HIP(w, hipSetDevice(home));
        sl.host.reset(); sl.body_cap = sl.ev_cap = 0;
        W_HIP(w, sl.host.alloc((size_t)body_cap * sizeof(edynhip_body_record) + (size_t)ev_cap * sizeof(ContactEvent), hipHostMallocPortable | hipHostMallocMapped));
        sl.body_cap = body_cap; sl.ev_cap = ev_cap;
    }
    size_t reported = 0;
    for (Shard &s : w->shards) {   // every shard's pack on its own stream, behind its last step and its event append
        if (!s.ctx || s.local_ids.empty()) continue;
        W_HIP(w, hipSetDevice(s.device));
        if (!s.res.rec_ev[k]) W_HIP(w, s.res.rec_ev[k].create(hipEventDisableTiming));
        void *dst = nullptr;
        W_HIP(w, hipHostGetDevicePointer(&dst, sl.host, 0));
        const int rc = shard_pack_records(s.ctx, s.res.ids_dev, (uint32_t)s.local_ids.size(), n, present_dt, dst);
        if (rc != EDYNHIP_OK) return w->fail(rc, std::string("edynhip_world_snapshot_records: ") + edynhip_last_error(s.ctx));
        W_HIP(w, hipEventRecord(s.res.rec_ev[k], s.ctx->stream));
        s.res.rec_pending[k] = true;
        reported += s.owned_local.size();
    }
    if (copy) {   // the event block: one copy from the home device's list, after every shard's append
        W_HIP(w, hipSetDevice(home));
        if (!w->rec_stream) W_HIP(w, w->rec_stream.create(hipStreamNonBlocking));
        if (!w->rec_ev_done[k]) W_HIP(w, w->rec_ev_done[k].create(hipEventDisableTiming));
        for (Shard &s : w->shards) if (s.res.rec_pending[k]) W_HIP(w, hipStreamWaitEvent(w->rec_stream, s.res.rec_ev[k], 0));
        W_HIP(w, hipMemcpyAsync(sl.host + (size_t)sl.body_cap * sizeof(edynhip_body_record), w->ev_list.h, (size_t)copy * sizeof(ContactEvent), hipMemcpyDeviceToHost, w->rec_stream));
        W_HIP(w, hipEventRecord(w->rec_ev_done[k], w->rec_stream));
        sl.ev_pending = true;
    }
    if (reported != n) {   // a body no shard reports (every shard reports a body at most once): the world writes its record
        std::vector<uint8_t> seen(n, 0);
        for (const Shard &s : w->shards) if (s.ctx) for (uint32_t l : s.owned_local) seen[s.local_ids[l]] = 1;
        for (uint32_t g = 0; g < n; ++g) if (!seen[g]) host_record(w, g, present_dt, ((edynhip_body_record *)(uint8_t *)sl.host)[g]);
    }
    sl.bodies = n; sl.step = w->step_count; sl.events = copy;
    sl.total = w->events_on() ? (uint32_t)std::min<uint64_t>(w->ev_occurred, 0xFFFFFFFFull) : 0u;
    sl.tombs = (uint32_t)w->tombs.size();
    w->rec_last = k;
    return EDYNHIP_OK;
}

int edynhip_world_snapshot_map(edynhip_world *w, edynhip_record_view *view) {
    if (!w || !view) return EDYNHIP_ERR_INVALID;
    if (w->rec_last < 0) return w->fail(EDYNHIP_ERR_INVALID, "edynhip_world_snapshot_map: no record snapshot was taken");
    const int k = w->rec_last;
    edynhip_world::RecSlot &sl = w->rec[k];
    EH_TRY(rec_wait(w, k));   // that snapshot only
    edynhip_body_record *rec = (edynhip_body_record *)(uint8_t *)sl.host;
    // a context rebuilt after the step that dropped a removed body holds the slot as a plain shapeless static body: the tombstone is the world's
    for (uint32_t t = 0; t < sl.tombs && t < w->tombs.size(); ++t) if (w->tombs[t] < sl.bodies) rec[w->tombs[t]].flags |= EDYNHIP_RECORD_REMOVED;
    view->records = rec;
    view->num_bodies = sl.bodies;
    view->step_index = sl.step;
    view->events = w->events_on() ? (const edynhip_contact_event *)(sl.host + (size_t)sl.body_cap * sizeof(edynhip_body_record)) : nullptr;
    view->num_events = sl.events;
    view->total_events = sl.total;
    return EDYNHIP_OK;
}

}  // extern "C"
