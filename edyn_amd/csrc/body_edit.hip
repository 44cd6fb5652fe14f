// C-ABI, bodies of a running world edited in place (include/edynhip.h edynhip_edit_bodies): set_rigidbody_mass / _inertia / _friction,
// rigidbody_set_shape and rigidbody_set_kind (util/rigidbody.cpp:300-362, :471-495, :579-606) as a few writes on the device instead of
// a fresh upload. Three pieces: k_edit_bodies, one lane per edited body, with the derivations of the upload (dbodyinit.hpp);
// k_edit_friction over the manifolds of the edited bodies; and the manifold drop of a SHAPE or KIND edit - the manifolds of the marked
// bodies leave the sorted array through a stable compaction into the other manifold buffer (k_drop_count, a scan of the block sums,
// k_drop_move, k_drop_segments). What the host refuses is ctx_rules.hpp's (validate_body_edit), what the edit invalidates ctx.hpp's.
#include "ctx.hpp"
#include "ctx_rules.hpp"
#include "dbodyinit.hpp"
#include <algorithm>
#include <cstring>

namespace eh {
using namespace dm;

static_assert(kPointRecords, "k_drop_move moves a manifold's points as one 320-byte record");
constexpr uint32_t kDropBlock = 256;                          // manifolds per workgroup of the drop kernels
constexpr uint32_t kRecordF = (uint32_t)kMaxPts * kPointF;    // float4 per point record

// One edited body as the host packs it (24 words): only the members of the named groups hold anything
struct EditRec {
    uint32_t index; int32_t kind, shape_type; uint32_t bits;   // bits: 1 = inertia given, 2 = gravity given
    float mass, friction, restitution, pad;
    float shape_param[4], inertia[9], gravity[3];
};
static_assert(sizeof(EditRec) == 96, "EditRec is staged as 24 words");

__global__ void k_edit_bodies(uint32_t n, const EditRec *__restrict__ recs, Bodies b, uint32_t fields, float3 default_gravity, dc::Meshes meshes,
                              uint32_t *mark, double *since) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const EditRec r = recs[t];
    const uint32_t i = r.index;
    uint32_t fl = b.flags[i];
    const int old_kind = (int)(fl & BF_KIND_MASK);
    const int kind = (fields & EDYNHIP_EDIT_KIND) ? r.kind : old_kind;
    int st = (int)((fl & BF_SHAPE_MASK) >> BF_SHAPE_SHIFT);
    float4 sp = b.shape[i];
    if (fields & EDYNHIP_EDIT_SHAPE) { st = r.shape_type; sp = make_float4(r.shape_param[0], r.shape_param[1], r.shape_param[2], r.shape_param[3]); }
    const q4 orn = q_from4(B_ORN(b, i));
    const f3 org = B_ORG(b, i);
    float4 p4 = B_POS(b, i);
    if (mark) mark[i] = 1u;
    if (kind == EDYNHIP_KIND_DYNAMIC) {   // (inverse mass and inertias of the others read 0, as after an upload)
        if (fields & EDYNHIP_EDIT_MASS) p4.w = 1.0f / r.mass;
        if (fields & EDYNHIP_EDIT_INERTIA) {
            const bool has_com = b.com && b.com[i].w != 0.0f;
            const f3 com = has_com ? from4(b.com[i]) : mk3(0, 0, 0);
            const m3 il = local_inertia_inv((r.bits & 1u) ? r.inertia : nullptr, st, sp, r.mass, com, has_com, meshes);
            const m3 iw = world_inertia_inv(il, orn);
            B_IW(b, i, 0) = to4(iw.r0, 0); B_IW(b, i, 1) = to4(iw.r1, 0); B_IW(b, i, 2) = to4(iw.r2, 0);
            B_IL(b, i, 0) = to4(il.r0, 0); B_IL(b, i, 1) = to4(il.r1, 0); B_IL(b, i, 2) = to4(il.r2, 0);
        }
    }
    if (fields & EDYNHIP_EDIT_KIND) {
        if (kind != EDYNHIP_KIND_DYNAMIC) {
            p4.w = 0;
            for (int k = 0; k < 3; ++k) { B_IW(b, i, k) = make_float4(0, 0, 0, 0); B_IL(b, i, k) = make_float4(0, 0, 0, 0); }
            b.grav[i] = make_float4(0, 0, 0, 0);
            B_DV(b, i) = make_float4(0, 0, 0, 0); B_DW(b, i) = make_float4(0, 0, 0, 0);
            if (kind == EDYNHIP_KIND_STATIC) { b.linvel[i] = make_float4(0, 0, 0, 0); b.angvel[i] = make_float4(0, 0, 0, 0); }
        } else {
            b.grav[i] = (r.bits & 2u) ? make_float4(r.gravity[0], r.gravity[1], r.gravity[2], 0) : make_float4(default_gravity.x, default_gravity.y, default_gravity.z, 0);
            if (old_kind != EDYNHIP_KIND_DYNAMIC) { b.island[i] = i; since[i] = -1.0; }   // an island of its own until the next step labels it, no timer
        }
        fl = (fl & ~BF_KIND_MASK) | (uint32_t)kind;
    }
    if (fields & (EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND)) fl &= ~BF_ASLEEP;
    if (fields & EDYNHIP_EDIT_SHAPE) {
        fl = (fl & ~BF_SHAPE_MASK) | ((uint32_t)st << BF_SHAPE_SHIFT);
        b.shape[i] = sp;
        f3 mn, mx;
        shape_aabb(st, sp, org, orn, meshes, mn, mx);
        b.amin[i] = to4(mn, 0); b.amax[i] = to4(mx, 0);
    }
    if (fields & EDYNHIP_EDIT_MATERIAL) b.mat[i] = make_float2(r.friction, r.restitution);
    B_POS(b, i) = p4;
    b.flags[i] = fl;
}

// set_rigidbody_friction's walk over the body's manifolds (rigidbody.cpp:329-361): one lane per manifold, the others stand down
__global__ void k_edit_friction(uint32_t M, Manifolds mf, Bodies b, const uint32_t *__restrict__ mark) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t ia = mf.bodyA[m], ib = mf.bodyB[m];
    if (!(mark[ia] | mark[ib])) return;
    float friction, restitution;
    if (mix_point_material(b, ia, ib, b.mat[ia], b.mat[ib], friction, restitution)) return;   // combined by the mix table: the points keep theirs
    const uint32_t np = mf.info[m] & 0xFFu;
    for (uint32_t k = 0; k < np; ++k) mf.pB[pt_at(mf.cap, k, m)].w = friction;
}

// ---- the manifold drop. misc[0]: highest colour in use among the manifolds that stay, + 1
// Pass 1: who stays (neither body marked), per workgroup the number that stay; the islands of the bodies that lose a manifold are marked
// for waking; the events of the manifolds that go. Event slots are taken with one atomic per wave.
__global__ void __launch_bounds__(kDropBlock)
k_drop_count(uint32_t M, Manifolds mf, Bodies b, const uint32_t *__restrict__ mark, uint32_t *bsum, uint32_t *misc, uint32_t *wake, EventSink ev) {
    __shared__ uint32_t w_keep[kDropBlock / 64], w_col[kDropBlock / 64];
    const uint32_t m = blockIdx.x * kDropBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool in = m < M;
    uint32_t ia = 0, ib = 0, info = 0;
    bool keep = false;
    if (in) { ia = mf.bodyA[m]; ib = mf.bodyB[m]; info = mf.info[m]; keep = !(mark[ia] | mark[ib]); }
    const bool drop = in && !keep;
    const uint32_t np = info & 0xFFu, colour = info >> 8;
    uint32_t col = (keep && np > 0 && colour != kNoColour) ? colour + 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) col = max(col, (uint32_t)__shfl_xor((int)col, off));
    const uint64_t kmask = __ballot(keep);
    if (lane == 0) { w_keep[wave] = (uint32_t)__popcll(kmask); w_col[wave] = col; }
    if (drop && wake) {
        if ((b.flags[ia] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) wake[b.island[ia]] = 1u;
        if ((b.flags[ib] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) wake[b.island[ib]] = 1u;
    }
    if (ev.buf) {   // per dropped manifold: its living points, then the manifold
        const uint32_t mine = drop ? np + 1u : 0u;
        uint32_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, d); if ((int)lane >= d) inc += u; }
        const uint32_t total = (uint32_t)__shfl((int)inc, 63);
        uint32_t base = 0;
        if (lane == 63 && total) base = atomicAdd(ev.count, total);   // may run past cap: the host reports the overflow
        base = (uint32_t)__shfl((int)base, 63);
        if (drop) {
            uint32_t at = base + inc - mine;
            for (uint32_t k = 0; k < np; ++k, ++at)
                if (at < ev.cap) ev.buf[at] = ContactEvent{EDYNHIP_EVENT_POINT_DESTROYED, ev.step, ia, ib, mf.pid[slot_at(mf.cap, k, m)]};
            if (at < ev.cap) ev.buf[at] = ContactEvent{EDYNHIP_EVENT_MANIFOLD_DESTROYED, ev.step, ia, ib, 0};
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0, c = 0;
        for (uint32_t w = 0; w < kDropBlock / 64; ++w) { s += w_keep[w]; c = max(c, w_col[w]); }
        bsum[blockIdx.x] = s;
        if (c) atomicMax(&misc[0], c);   // (one per workgroup)
    }
}
// Pass 2: the manifolds that stay move to their places in the other buffer, in order (boff: exclusive scan of bsum). The per-manifold
// arrays are written by the manifold's lane - consecutive lanes, consecutive places; the 320-byte point records by the whole workgroup,
// 16 bytes per lane and contiguous in the destination. tree starts at 0 as after edynhip_set_manifolds (the forced relabel rebuilds
// the certificate); a polyhedron pair's separating-axis hint goes with its manifold.
__global__ void __launch_bounds__(kDropBlock)
k_drop_move(uint32_t M, Manifolds src, Manifolds dst, const uint32_t *__restrict__ mark, const uint32_t *__restrict__ boff,
            const uint32_t *__restrict__ hint_src, uint32_t *hint_dst) {
    __shared__ uint32_t w_keep[kDropBlock / 64], s_src[kDropBlock];
    const uint32_t m = blockIdx.x * kDropBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool keep = false;
    if (m < M) keep = !(mark[src.bodyA[m]] | mark[src.bodyB[m]]);
    const uint64_t kmask = __ballot(keep);
    if (lane == 0) w_keep[wave] = (uint32_t)__popcll(kmask);
    __syncthreads();
    uint32_t local = (uint32_t)__popcll(kmask & ((1ull << lane) - 1ull)), kept = 0;
    for (uint32_t w = 0; w < kDropBlock / 64; ++w) { if (w < wave) local += w_keep[w]; kept += w_keep[w]; }
    const uint32_t base = boff[blockIdx.x];
    if (keep) {
        const uint32_t d = base + local;   // (d <= m < cap)
        s_src[local] = m;
        dst.skey[d] = src.skey[m]; dst.bodyA[d] = src.bodyA[m]; dst.bodyB[d] = src.bodyB[m];
        const uint32_t info = src.info[m];
        dst.info[d] = info;
        dst.tree[d] = 0;
        dst.prev_idx[d] = 0xFFFFFFFFu;
        if (hint_dst) hint_dst[d] = hint_src[m];
        const uint32_t np = info & 0xFFu;
        for (uint32_t k = 0; k < np; ++k) {
            const size_t s = slot_at(src.cap, k, m), t = slot_at(dst.cap, k, d);
            if (dst.pid) dst.pid[t] = src.pid[s];
            if (dst.xmat) { dst.xmat[t] = src.xmat[s]; dst.ximp[t] = src.ximp[s]; }
        }
    }
    __syncthreads();
    const float4 *__restrict__ from = src.pA;
    float4 *to = dst.pA + (size_t)base * kRecordF;
    for (uint32_t e = threadIdx.x; e < kept * kRecordF; e += kDropBlock) {
        const uint32_t rec = e / kRecordF, piece = e - rec * kRecordF;
        to[e] = from[(size_t)s_src[rec] * kRecordF + piece];
    }
}
// Pass 3: the owners' segments of the new array, as k_bp_build_manifolds leaves them (seg_start / seg_end were cleared)
__global__ void k_drop_segments(const uint32_t *__restrict__ total, Manifolds dst) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x, M = *total;
    if (m >= M) return;
    const uint32_t hi = (uint32_t)(dst.skey[m] >> 33);
    const uint32_t ph = m > 0 ? (uint32_t)(dst.skey[m - 1] >> 33) : 0xFFFFFFFFu;
    const uint32_t nh = m + 1 < M ? (uint32_t)(dst.skey[m + 1] >> 33) : 0xFFFFFFFFu;
    if (ph != hi) dst.seg_start[hi] = m;
    if (nh != hi) dst.seg_end[hi] = m + 1;
}

// The edit itself: what edynhip_edit_bodies does on its context, and what a multi-device world does on the shard(s) that hold the bodies
// (multi_body_edit.hip, local indices).
int edit_bodies(edynhip_ctx *c, uint32_t n, const uint32_t *indices, const edynhip_bodies *in, uint32_t fields) {
    {
        const char *why = "";
        const int rc = validate_body_edit(n, indices, in, fields, c->b.n, c->host_removed, (uint32_t)c->host_meshes.desc.size(), &why);
        if (rc != EDYNHIP_OK) return set_error(c, rc, (std::string("edynhip_edit_bodies: ") + why).c_str());
    }
    if (n == 0 || fields == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const bool reshape = fields & EDYNHIP_EDIT_SHAPE, rekind = fields & EDYNHIP_EDIT_KIND, drops = reshape || rekind;
    const bool marks = drops || (fields & EDYNHIP_EDIT_MATERIAL);
    const uint32_t M = c->num_manifolds, nb = c->b.n;

    // the bodies that share a joint with an edited one wake with it; the joints of a body whose kind changes are coloured again
    std::vector<uint32_t> partners;
    bool joints_touched = false;
    if (drops && !c->host_joints.empty()) {
        EH_TRY(flush_joint_redefs(c));
        std::vector<uint32_t> sorted(indices, indices + n);
        std::sort(sorted.begin(), sorted.end());
        for (const HostJoint &h : c->host_joints)
            if (h.alive && (std::binary_search(sorted.begin(), sorted.end(), h.body[0]) || std::binary_search(sorted.begin(), sorted.end(), h.body[1]))) {
                partners.push_back(h.body[0]); partners.push_back(h.body[1]);
                joints_touched = true;
            }
    }
    if (reshape)   // (may grow the rotated-mesh buffer)
        for (uint32_t k = 0; k < n; ++k)
            if (in->shape_type[k] == EDYNHIP_SHAPE_POLYHEDRON) EH_TRY(mesh_bind_body(c, indices[k], (uint32_t)in->shape_param[4 * (size_t)k]));

    // one buffer, no allocation per call: [marks: bodies][misc: 4][bsum: blocks + 1][boff: blocks + 1][wake list][records]
    const uint32_t nblk = drops ? blocks(M, kDropBlock) : 0u;
    const size_t n_list = drops && c->sleeping ? (size_t)n + partners.size() : 0;
    const size_t o_misc = marks ? nb : 0, o_bsum = o_misc + 4, o_boff = o_bsum + nblk + 1, o_list = o_boff + nblk + 1, o_recs = o_list + n_list;
    uint32_t *scratch = nullptr;
    EH_TRY(index_scratch(c, o_recs + (size_t)n * (sizeof(EditRec) / sizeof(uint32_t)), scratch));
    uint32_t *mark = marks ? scratch : nullptr, *misc = scratch + o_misc, *bsum = scratch + o_bsum, *boff = scratch + o_boff, *list = scratch + o_list;
    EditRec *recs_dev = (EditRec *)(scratch + o_recs);
    std::vector<EditRec> recs(n);
    for (uint32_t k = 0; k < n; ++k) {
        EditRec &r = recs[k];
        std::memset(&r, 0, sizeof(r));
        r.index = indices[k];
        if (fields & EDYNHIP_EDIT_MASS) r.mass = in->mass[k];
        if ((fields & EDYNHIP_EDIT_INERTIA) && in->has_inertia && in->has_inertia[k]) { r.bits |= 1u; std::memcpy(r.inertia, in->inertia + 9 * (size_t)k, sizeof(r.inertia)); }
        if (fields & EDYNHIP_EDIT_MATERIAL) { r.friction = in->friction[k]; r.restitution = in->restitution[k]; }
        if (reshape) { r.shape_type = in->shape_type[k]; std::memcpy(r.shape_param, in->shape_param + 4 * (size_t)k, sizeof(r.shape_param)); }
        if (rekind) { r.kind = in->kind[k]; if (in->gravity) { r.bits |= 2u; std::memcpy(r.gravity, in->gravity + 3 * (size_t)k, sizeof(r.gravity)); } }
    }
    EH_HIP(c, hipMemsetAsync(scratch, 0, (o_bsum + nblk + 1) * sizeof(uint32_t), s));   // marks, misc, and bsum's closing 0
    EH_HIP(c, hipMemcpyAsync(recs_dev, recs.data(), recs.size() * sizeof(EditRec), hipMemcpyHostToDevice, s));
    const bool waking = drops && c->sleeping;
    if (waking) {   // the islands the edited bodies and their joint partners are in now, by the rule of edynhip_remove_bodies
        std::vector<uint32_t> touched(indices, indices + n);
        touched.insert(touched.end(), partners.begin(), partners.end());
        EH_HIP(c, hipMemcpyAsync(list, touched.data(), touched.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        EH_HIP(c, hipStreamSynchronize(s));   // (`touched` is a local)
        EH_HIP(c, hipMemsetAsync(c->sleep_action, 0, (size_t)nb * sizeof(uint32_t), s));
        mark_islands_of(c, (uint32_t)touched.size(), list);
    }
    hipLaunchKernelGGL(k_edit_bodies, dim3(blocks(n, 64)), dim3(64), 0, s, n, recs_dev, c->b, fields,
                       make_float3(c->cfg.gravity[0], c->cfg.gravity[1], c->cfg.gravity[2]), c->meshes, mark, c->sleep_since);
    uint32_t kept = M, top = 0;
    if (drops && M > 0) {
        const Manifolds &from = c->m[c->cur], &to = c->m[c->cur ^ 1];
        uint32_t *hints = c->poly_work ? c->poly_work + 3 * 1024 + 1 + 2 * (size_t)from.cap : nullptr;   // narrowphase.hip PolyBins: [2][cap], one array per manifold buffer
        EH_HIP(c, hipMemsetAsync(to.seg_start, 0, (size_t)c->b.cap * sizeof(uint32_t), s));
        EH_HIP(c, hipMemsetAsync(to.seg_end, 0, (size_t)c->b.cap * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_drop_count, dim3(nblk), dim3(kDropBlock), 0, s, M, from, c->b, mark, bsum, misc, waking ? c->sleep_action : nullptr, event_sink(c));
        EH_TRY(scan_u32(c, bsum, boff, nblk + 1));
        hipLaunchKernelGGL(k_drop_move, dim3(nblk), dim3(kDropBlock), 0, s, M, from, to, mark, boff,
                           hints ? hints + (size_t)c->cur * from.cap : nullptr, hints ? hints + (size_t)(c->cur ^ 1) * from.cap : nullptr);
        hipLaunchKernelGGL(k_drop_segments, dim3(blocks(M, 256)), dim3(256), 0, s, boff + nblk, to);
        EH_HIP(c, hipMemcpyAsync(&kept, boff + nblk, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        EH_HIP(c, hipMemcpyAsync(&top, misc, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    } else if ((fields & EDYNHIP_EDIT_MATERIAL) && M > 0) {
        hipLaunchKernelGGL(k_edit_friction, dim3(blocks(M, 256)), dim3(256), 0, s, M, c->m[c->cur], c->b, mark);
    }
    if (waking) wake_marked_islands(c);
    {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);   // the staged records are locals; the scratch may be refilled by the next call
        if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_edit_bodies", e);
    }
    // ---- host facts
    const bool dropped = kept != M;
    if (dropped) {   // the compacted array is the current one; the colours in use as edynhip_set_manifolds counts them
        c->cur ^= 1;
        c->num_manifolds = kept;
        c->num_colours = top;
        c->points_in_prev = false;
    }
    if (fields & EDYNHIP_EDIT_MATERIAL)
        for (uint32_t k = 0; k < n; ++k) if (in->restitution[k] > 0.0f) c->has_restitution = true;   // turns the restitution solver on (restitution.hip)
    bool set_changed = false, kind_changed = false;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = indices[k];
        const int32_t old_kind = c->host_kind[i], old_shape = c->host_shape[i];
        const int32_t kind = rekind ? in->kind[k] : old_kind, shape = reshape ? in->shape_type[k] : old_shape;
        const bool was_proc = old_kind == EDYNHIP_KIND_DYNAMIC, is_proc = kind == EDYNHIP_KIND_DYNAMIC;
        set_changed = set_changed || was_proc != is_proc || (old_shape == EDYNHIP_SHAPE_NONE) != (shape == EDYNHIP_SHAPE_NONE);
        kind_changed = kind_changed || kind != old_kind;
        if (was_proc != is_proc && !c->host_nosleep[i]) c->num_sleepable += is_proc ? 1u : 0xFFFFFFFFu;
        c->host_kind[i] = kind; c->host_shape[i] = shape;
    }
    if (reshape) {   // the narrowphase's extra kernels follow the shapes in use
        c->has_cylinder = false;
        bool poly = false;
        for (uint32_t i = 0; i < nb; ++i) { c->has_cylinder = c->has_cylinder || c->host_shape[i] == EDYNHIP_SHAPE_CYLINDER; poly = poly || c->host_shape[i] == EDYNHIP_SHAPE_POLYHEDRON; }
        c->has_polyhedron = poly;
    }
    if (set_changed) EH_TRY(rebuild_broadphase_lists(c));
    if (kind_changed && joints_touched) EH_TRY(rebuild_joints(c, true));   // the joints' colouring reads who is dynamic
    invalidate_bodies_edited(c, reshape, rekind, dropped);
    return EDYNHIP_OK;
}

}  // namespace eh

using namespace eh;

extern "C" {

int edynhip_edit_bodies(edynhip_ctx *c, uint32_t n, const uint32_t *indices, const edynhip_bodies *in, uint32_t fields) {
    if (!c) return EDYNHIP_ERR_INVALID;
    if (c->world_shard) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, "edynhip_edit_bodies: a shard of a multi-device world takes its bodies from the world");
    return edit_bodies(c, n, indices, in, fields);
}

}  // extern "C"
