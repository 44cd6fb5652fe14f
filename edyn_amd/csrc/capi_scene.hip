// C-ABI, scene edits (include/edynhip.h): body upload, add and removal, the host joint list and its device arrays, exclusions and the
// pair filter, contact_extras materials and the mix table, centre-of-mass edits, parameters and gravity, sleep and wake edits.
// Host-side logic and the small kernels the edits need; the rules with content of their own are ctx_rules.hpp's, what an edit
// invalidates is ctx.hpp's (invalidate_*).
#include "ctx.hpp"
#include "ctx_rules.hpp"
#include "dstep.hpp"
#include "dpolyhedron.hpp"
#include "dbodyinit.hpp"
#include <algorithm>
#include <cstring>

namespace eh {
using namespace dm;

static_assert(kJointNoColour == kNoColour && kJointMaxColours == kMaxColours && kExclCap == 16, "ctx_rules.hpp mirrors ctx.hpp");

// Scene upload: raw packed arrays -> float4 SoA + derived quantities (rigidbody.cpp:47-131).
struct RawBodies {
    const int32_t *kind; const float *pos, *orn, *linvel, *angvel, *mass, *inertia; const uint8_t *has_inertia;
    const int32_t *shape_type; const float *shape_param, *friction, *restitution; const uint64_t *group, *mask; const float *gravity; const uint8_t *sleeping_disabled; const float *com;
};
__global__ void k_init_bodies(uint32_t first, uint32_t n, RawBodies r, Bodies b, float3 default_gravity, dc::Meshes meshes) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;   // index into the caller's arrays
    if (l >= n) return;
    const uint32_t i = first + l;                                // body index
    const int kind = r.kind[l], st = r.shape_type[l];
    const f3 pos = mk3(r.pos[3 * l], r.pos[3 * l + 1], r.pos[3 * l + 2]);
    const q4 orn{r.orn[4 * l], r.orn[4 * l + 1], r.orn[4 * l + 2], r.orn[4 * l + 3]};
    const float4 sp = make_float4(r.shape_param[4 * l], r.shape_param[4 * l + 1], r.shape_param[4 * l + 2], r.shape_param[4 * l + 3]);
    float inv_m = 0;
    m3 il = m3_zero(), iw = m3_zero();
    const f3 com = r.com ? mk3(r.com[3 * l], r.com[3 * l + 1], r.com[3 * l + 2]) : mk3(0, 0, 0);
    const bool has_com = !(com.x == 0 && com.y == 0 && com.z == 0);
    if (kind == EDYNHIP_KIND_DYNAMIC) {
        const float mass = r.mass[l];
        inv_m = 1.0f / mass;
        il = local_inertia_inv((r.has_inertia && r.has_inertia[l]) ? r.inertia + 9 * l : nullptr, st, sp, mass, com, has_com, meshes);
        iw = world_inertia_inv(il, orn);
    }
    const bool moving = kind != EDYNHIP_KIND_STATIC;
    f3 lv = moving ? mk3(r.linvel[3 * l], r.linvel[3 * l + 1], r.linvel[3 * l + 2]) : mk3(0, 0, 0);
    const f3 av = moving ? mk3(r.angvel[3 * l], r.angvel[3 * l + 1], r.angvel[3 * l + 2]) : mk3(0, 0, 0);
    f3 pos_com = pos;
    if (has_com) {   // apply_center_of_mass (rigidbody.cpp:517-548): the given position is the origin
        pos_com = to_world(com, pos, orn);
        if (moving) lv += cross(av, pos_com - pos);
    }
    if (b.com) { b.com[i] = to4(com, has_com ? 1.0f : 0.0f); b.origin[i] = to4(pos, 0); }
    B_POS(b, i) = to4(pos_com, inv_m);
    B_ORN(b, i) = to4(orn);
    b.linvel[i] = to4(lv, 0);
    b.angvel[i] = to4(av, 0);
    B_DV(b, i) = make_float4(0, 0, 0, 0); B_DW(b, i) = make_float4(0, 0, 0, 0);
    B_IW(b, i, 0) = to4(iw.r0, 0); B_IW(b, i, 1) = to4(iw.r1, 0); B_IW(b, i, 2) = to4(iw.r2, 0);
    B_IL(b, i, 0) = to4(il.r0, 0); B_IL(b, i, 1) = to4(il.r1, 0); B_IL(b, i, 2) = to4(il.r2, 0);
    b.shape[i] = sp;
    f3 g = r.gravity ? mk3(r.gravity[3 * l], r.gravity[3 * l + 1], r.gravity[3 * l + 2]) : mk3(default_gravity.x, default_gravity.y, default_gravity.z);
    b.grav[i] = kind == EDYNHIP_KIND_DYNAMIC ? to4(g, 0) : make_float4(0, 0, 0, 0);
    b.mat[i] = make_float2(r.friction[l], r.restitution[l]);
    b.mat2[i] = make_float4(0.0f, 0.0f, kLarge, kLarge);   // material defaults (comp/material.hpp:15-22); edynhip_set_material_extras changes them
    b.flags[i] = (uint32_t)kind | ((uint32_t)st << BF_SHAPE_SHIFT) | ((r.sleeping_disabled && r.sleeping_disabled[l]) ? BF_NOSLEEP : 0u);
    b.group[i] = r.group ? r.group[l] : ~0ull;
    b.mask[i] = r.mask ? r.mask[l] : ~0ull;
    b.island[i] = i;
    f3 mn, mx;
    shape_aabb(st, sp, pos, orn, meshes, mn, mx);
    b.amin[i] = to4(mn, 0); b.amax[i] = to4(mx, 0);
}

// One of the caller's arrays on the device for the length of an upload: `tmp` owns the copies
template <typename T>
static int upload(edynhip_ctx *c, const T *host, size_t count, const T *&dev, std::vector<DeviceBuf<uint8_t>> &tmp) {
    dev = nullptr;
    if (!host || count == 0) return EDYNHIP_OK;
    tmp.emplace_back();
    EH_HIP(c, tmp.back().alloc(count * sizeof(T)));
    EH_HIP(c, hipMemcpyAsync(tmp.back(), host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    dev = (const T *)(uint8_t *)tmp.back();
    return EDYNHIP_OK;
}

// ---- removal (registry.destroy on a rigid body: island_manager.cpp:47-115)
__global__ void k_mark_removed(uint32_t n, const uint32_t *__restrict__ list, Bodies b, uint32_t *wake) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = list[t];
    const uint32_t fl = b.flags[i];
    if ((fl & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) wake[b.island[i]] = 1u;
    b.flags[i] = EDYNHIP_KIND_STATIC | BF_REMOVED;     // shapeless, static, awake: no stage touches it any more
    b.linvel[i] = make_float4(0, 0, 0, 0); b.angvel[i] = make_float4(0, 0, 0, 0);
    b.grav[i] = make_float4(0, 0, 0, 0);
    float4 p = B_POS(b, i); p.w = 0; B_POS(b, i) = p;
    B_DV(b, i) = make_float4(0, 0, 0, 0); B_DW(b, i) = make_float4(0, 0, 0, 0);
    b.island[i] = i;
}
__global__ void k_mark_touching(uint32_t n, const uint32_t *__restrict__ list, Bodies b, uint32_t *wake) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t i = list[t];
    if ((b.flags[i] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) wake[b.island[i]] = 1u;
}
__global__ void k_wake_partners(uint32_t M, Manifolds mf, Bodies b, uint32_t *wake) {   // islands resting on a removed static/kinematic body
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const uint32_t a = mf.bodyA[m], bb = mf.bodyB[m];
    const bool ra = b.flags[a] & BF_REMOVED, rb = b.flags[bb] & BF_REMOVED;
    if (ra && (b.flags[bb] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) wake[b.island[bb]] = 1u;
    if (rb && (b.flags[a] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) wake[b.island[a]] = 1u;
}
// restart: the island's sleep timer starts again as well (an edit of the body itself). wake_up_island (util/island_util.cpp:61-66) alone only takes
// the sleeping tags off: the timer of an awake island that loses a joint or a body, or is woken by the caller, goes on running.
__global__ void k_wake_marked(uint32_t n, Bodies b, uint32_t *wake, double *since, bool restart) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t fl = b.flags[i];
    if ((fl & BF_KIND_MASK) != EDYNHIP_KIND_DYNAMIC) return;
    const uint32_t l = b.island[i];
    if (wake[l]) { b.flags[i] = fl & ~BF_ASLEEP; if (restart && l == i) since[i] = -1.0; }
}
// Index lists handed to small kernels (bodies to wake, bodies to remove): one persistent device buffer that grows on demand
// and is released with the context - no hipMalloc / hipFree per call, nothing to leak on an error path.
int index_scratch(edynhip_ctx *c, size_t count, uint32_t *&out) {
    IndexScratch &s = c->idx_scratch;
    if (count > s.cap) {
        s.cap = 0;
        const size_t cap = std::max<size_t>(count * 2, 1024);
        EH_HIP(c, s.buf.alloc(cap));
        s.cap = cap;
    }
    out = s.buf;
    return EDYNHIP_OK;
}
// The two halves of a wake-up for callers that mark more islands in between (body_edit.hip): sleep_action[label] = 1 for the islands of
// the listed bodies (device list; the caller cleared sleep_action), and every dynamic body of a marked island awake, its timer restarted
void mark_islands_of(edynhip_ctx *c, uint32_t n, const uint32_t *list_dev) {
    if (n) hipLaunchKernelGGL(k_mark_touching, dim3(blocks(n, 128)), dim3(128), 0, c->stream, n, list_dev, c->b, c->sleep_action);
}
void wake_marked_islands(edynhip_ctx *c) {
    if (c->b.n) hipLaunchKernelGGL(k_wake_marked, dim3(blocks(c->b.n, 256)), dim3(256), 0, c->stream, c->b.n, c->b, c->sleep_action, c->sleep_since, true);
}
// wake the islands of the listed bodies (wake_up_island, island_manager.cpp:541-571)
int wake_islands_of(edynhip_ctx *c, const std::vector<uint32_t> &bodies) {
    if (!c->sleeping || bodies.empty() || c->b.n == 0) { invalidate_woke(c); return EDYNHIP_OK; }
    uint32_t *list = nullptr;
    EH_TRY(index_scratch(c, bodies.size(), list));
    EH_HIP(c, hipMemcpyAsync(list, bodies.data(), bodies.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipMemsetAsync(c->sleep_action, 0, (size_t)c->b.n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_mark_touching, dim3(blocks((uint32_t)bodies.size(), 128)), dim3(128), 0, c->stream, (uint32_t)bodies.size(), list, c->b, c->sleep_action);
    hipLaunchKernelGGL(k_wake_marked, dim3(blocks(c->b.n, 256)), dim3(256), 0, c->stream, c->b.n, c->b, c->sleep_action, c->sleep_since, false);
    hipError_t e = hipStreamSynchronize(c->stream);   // the scratch list may be refilled by the next call
    invalidate_woke(c);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "wake_islands_of", e);
    return EDYNHIP_OK;
}

// broadphase participants from the host mirror of (kind, shape): [shaped non-procedural ..., shaped procedural ...]
int rebuild_broadphase_lists(edynhip_ctx *c) {
    uint32_t num_np = 0;
    const std::vector<uint32_t> list = broadphase_participants(c->host_kind, c->host_shape, num_np);
    // only procedural shaped bodies own pairs; everybody else's count must read 0 in the scan
    EH_HIP(c, hipMemsetAsync(c->own_count, 0, ((size_t)c->b.cap + 1) * sizeof(uint32_t), c->stream));
    c->bvh.age = 0;   // the tree topology is rebuilt on the next step
    invalidate_body_set_changed(c);
    c->bvh.num_np = num_np;
    c->bvh.num_proc = (uint32_t)list.size() - num_np;
    if (!list.empty())
        EH_HIP(c, hipMemcpyAsync(c->bvh.np_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));   // the list (a local) must outlive the copy
    return EDYNHIP_OK;
}

static int rebuild_mix_table(edynhip_ctx *c);
static int load_bodies(edynhip_ctx *c, uint32_t first, uint32_t n, const edynhip_bodies *in, const char *who) {
    if (c) invalidate_topology_changed(c);
    if (!c || !in) return EDYNHIP_ERR_INVALID;
    if ((uint64_t)first + n > c->b.cap) return set_error(c, EDYNHIP_ERR_CAPACITY, (std::string(who) + ": more than max_bodies").c_str());
    if (n && (!in->kind || !in->pos || !in->orn || !in->linvel || !in->angvel || !in->mass || !in->shape_type || !in->shape_param ||
              !in->friction || !in->restitution))
        return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": missing array").c_str());
    for (uint32_t i = 0; i < n; ++i)
        if (in->shape_type[i] < EDYNHIP_SHAPE_NONE || in->shape_type[i] > EDYNHIP_SHAPE_POLYHEDRON)
            return set_error(c, EDYNHIP_ERR_UNSUPPORTED, (std::string(who) + ": shape type not on this path (box, sphere, plane, capsule, cylinder, polyhedron)").c_str());
    EH_HIP(c, hipSetDevice(c->device));   // before anything allocates: a process may hold contexts on several GPUs
    EH_TRY(mesh_bind_bodies(c, first, n, in->shape_type, in->shape_param));
    // whatever happens below, the next step starts from scratch (also when an upload fails half way)
    invalidate_contact_state_replaced(c);
    if (first == 0) c->has_cylinder = false;
    for (uint32_t i = 0; i < n; ++i) if (in->shape_type[i] == EDYNHIP_SHAPE_CYLINDER) c->has_cylinder = true;   // narrowphase.hip launches k_np_detect_ext
    if (first == 0) { c->has_restitution = false; c->extras = false; c->mix.mat_id.clear(); c->b.mix_K = 0; for (auto &kv : c->mix.host) if (kv.second[0] > 0) c->has_restitution = true; }
    for (uint32_t i = 0; i < n; ++i)
        if (in->restitution[i] > 0.0f) c->has_restitution = true;   // turns the restitution solver on (restitution.hip)
    if (first == 0) { c->host_joints.clear(); c->j.n = 0; c->j.num_colours = 0; c->j.rows = 0; c->exclusions.host.clear(); c->exclusions.dirty_lo = 0xFFFFFFFFu; c->exclusions.dirty_hi = 0; if (c->excl) (void)hipMemsetAsync(c->excl, 0xFF, (size_t)c->b.cap * 16 * sizeof(uint32_t), c->stream); }
    const uint32_t total = first + n;
    {
        std::vector<DeviceBuf<uint8_t>> tmp;   // the caller's arrays on the device, until k_init_bodies has read them
        RawBodies r{};
        EH_TRY(upload(c, in->kind, n, r.kind, tmp)); EH_TRY(upload(c, in->pos, (size_t)n * 3, r.pos, tmp)); EH_TRY(upload(c, in->orn, (size_t)n * 4, r.orn, tmp));
        EH_TRY(upload(c, in->linvel, (size_t)n * 3, r.linvel, tmp)); EH_TRY(upload(c, in->angvel, (size_t)n * 3, r.angvel, tmp)); EH_TRY(upload(c, in->mass, n, r.mass, tmp));
        EH_TRY(upload(c, in->inertia, in->has_inertia ? (size_t)n * 9 : 0, r.inertia, tmp)); EH_TRY(upload(c, in->has_inertia, in->inertia ? n : 0, r.has_inertia, tmp));
        EH_TRY(upload(c, in->shape_type, n, r.shape_type, tmp)); EH_TRY(upload(c, in->shape_param, (size_t)n * 4, r.shape_param, tmp));
        EH_TRY(upload(c, in->friction, n, r.friction, tmp)); EH_TRY(upload(c, in->restitution, n, r.restitution, tmp));
        EH_TRY(upload(c, in->group, n, r.group, tmp)); EH_TRY(upload(c, in->mask, n, r.mask, tmp)); EH_TRY(upload(c, in->gravity, (size_t)n * 3, r.gravity, tmp));
        {   // host mirror of the collision groups / masks (edynhip_default_should_collide)
            c->host_group.resize((size_t)first + n, ~0ull); c->host_mask.resize((size_t)first + n, ~0ull);
            for (uint32_t i = 0; i < n; ++i) { c->host_group[first + i] = in->group ? in->group[i] : ~0ull; c->host_mask[first + i] = in->mask ? in->mask[i] : ~0ull; }
        }
        EH_TRY(upload(c, in->sleeping_disabled, n, r.sleeping_disabled, tmp));
        if (first == 0) c->num_sleepable = 0;
        for (uint32_t i = 0; i < n; ++i) if (in->kind[i] == EDYNHIP_KIND_DYNAMIC && !(in->sleeping_disabled && in->sleeping_disabled[i])) ++c->num_sleepable;
        {   // centre-of-mass offsets: the origin arrays are attached to the body set with the first body that has one
            bool any = false;
            if (in->center_of_mass) for (size_t k = 0; k < (size_t)n * 3; ++k) any = any || in->center_of_mass[k] != 0.0f;
            if (first == 0) { c->b.com = nullptr; c->b.origin = nullptr; }
            if (any && !c->b.com) {
                if (first != 0 && hipMemsetAsync(c->com_store, 0, (size_t)c->b.cap * sizeof(float4), c->stream) != hipSuccess) return EDYNHIP_ERR_HIP;
                c->b.com = c->com_store; c->b.origin = c->origin_store;
            }
            if (c->b.com) EH_TRY(upload(c, in->center_of_mass, in->center_of_mass ? (size_t)n * 3 : 0, r.com, tmp));
        }
        c->b.n = total;
        c->stats.num_bodies = total;
        if (n)
            hipLaunchKernelGGL(k_init_bodies, dim3(blocks(n, 256)), dim3(256), 0, c->stream, first, n, r, c->b,
                               make_float3(c->cfg.gravity[0], c->cfg.gravity[1], c->cfg.gravity[2]), c->meshes);
        c->host_kind.resize(first); c->host_shape.resize(first);
        c->host_removed.resize(first, 0); c->host_removed.resize((size_t)first + n, 0); c->host_nosleep.resize(first, 0);   // (an upload holds no tombstones)
        for (uint32_t i = 0; i < n; ++i) c->host_nosleep.push_back(in->sleeping_disabled && in->sleeping_disabled[i] ? 1 : 0);
        c->host_kind.insert(c->host_kind.end(), in->kind, in->kind + n);
        c->host_shape.insert(c->host_shape.end(), in->shape_type, in->shape_type + n);
        EH_TRY(rebuild_broadphase_lists(c));
        if (first != 0 && c->b.mix_K) EH_TRY(rebuild_mix_table(c));   // appended bodies carry no material id yet
        (void)hipStreamSynchronize(c->stream);
    }
    if (first == 0) {   // a new world: no manifolds, no running sleep timers (appended bodies keep every index stable instead)
        c->num_manifolds = 0;
        c->prev_num_manifolds = 0;
        c->step_index = 0;
        c->num_colours = 0;
        (void)hipMemsetAsync(c->sleep_since, 0xFF, (size_t)c->b.cap * sizeof(double), c->stream);
        c->sim_clock = 0;
        (void)hipMemsetAsync(c->sleep_state, 0, (size_t)c->b.cap * sizeof(uint32_t), c->stream);
        (void)hipMemsetAsync(c->sleep_action, 0, (size_t)c->b.cap * sizeof(uint32_t), c->stream);
        (void)hipMemsetAsync(c->sleep_size, 0, (size_t)c->b.cap * sizeof(uint32_t), c->stream);
        (void)hipMemsetAsync(c->sleep_best, 0, (size_t)c->b.cap * sizeof(unsigned long long), c->stream);
        c->sleep_prev_n = 0;   // no islands of a previous step
        c->sleep_prev_joints = 0;
        c->island_labels_valid = false;
        (void)hipStreamSynchronize(c->stream);
    }
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

// Host joint list -> device arrays: deterministic edge colouring over the live joints in caller-index order (ctx_rules.hpp
// colour_joints), colour-sorted upload, applied impulses and hinge angles carried along.
// fetch = first read the current impulses / angles back from the device (the joints were stepped since the last rebuild).
int rebuild_joints(edynhip_ctx *c, bool fetch) {
    Joints &j = c->j;
    invalidate_topology_changed(c);
    hipStream_t s = c->stream;
    std::vector<HostJoint> &hj = c->host_joints;
    if (fetch && j.n) {
        std::vector<float> imp((size_t)j.cap * kJointSlots), ang(j.n);
        std::vector<uint32_t> orig(j.n);
        EH_HIP(c, hipMemcpyAsync(imp.data(), j.impulse, imp.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        EH_HIP(c, hipMemcpyAsync(ang.data(), j.angle, (size_t)j.n * sizeof(float), hipMemcpyDeviceToHost, s));
        EH_HIP(c, hipMemcpyAsync(orig.data(), j.orig, (size_t)j.n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        EH_HIP(c, hipStreamSynchronize(s));
        for (uint32_t p = 0; p < j.n; ++p) {
            HostJoint &h = hj[orig[p]];
            for (int r = 0; r < kJointSlots; ++r) h.impulse[r] = imp[(size_t)r * j.cap + p];
            h.angle = ang[p];
        }
    }
    std::vector<uint32_t> live;
    c->has_generic = false;
    for (uint32_t e = 0; e < hj.size(); ++e) if (hj[e].alive) { live.push_back(e); if (hj[e].type == EDYNHIP_JOINT_GENERIC) c->has_generic = true; }
    const uint32_t n = (uint32_t)live.size();
    if (n > j.cap) return set_error(c, EDYNHIP_ERR_CAPACITY, "joints: more live joints than max_joints");
    j.n = n; j.num_colours = 0; j.rows = 0;
    invalidate_graph_changed(c, true);
    std::memset(j.colour_start, 0, sizeof(j.colour_start));
    c->stats.num_joints = n; c->stats.num_joint_rows = 0; c->stats.num_joint_colours = 0;
    if (n == 0) return EDYNHIP_OK;
    std::vector<uint32_t> ends(2 * (size_t)n), colour, order;
    for (uint32_t e = 0; e < n; ++e) { ends[2 * e] = hj[live[e]].body[0]; ends[2 * e + 1] = hj[live[e]].body[1]; }
    std::vector<uint8_t> dynamic(c->b.n);
    for (uint32_t i = 0; i < c->b.n; ++i) dynamic[i] = c->host_kind[i] == EDYNHIP_KIND_DYNAMIC;
    if (!colour_joints(n, ends.data(), dynamic, colour)) return set_error(c, EDYNHIP_ERR_COLOURS, "joints: more than 64 joint colours");
    const uint32_t ncol = colour_sorted_order(colour, order, j.colour_start);
    std::vector<uint32_t> orig(n), type(n), bA(n), bB(n);
    std::vector<float4> pivA(n), pivB(n), axA(n), pA(n), qA(n), axB(n), pB(n);
    std::vector<float> params((size_t)j.cap * kJointParams, 0.0f), impulse((size_t)j.cap * kJointSlots, 0.0f), angle(n);
    uint32_t rows = 0;
    for (uint32_t p = 0; p < n; ++p) {
        const HostJoint &h = hj[live[order[p]]];
        orig[p] = live[order[p]];
        type[p] = (uint32_t)h.type; bA[p] = h.body[0]; bB[p] = h.body[1];
        pivA[p] = make_float4(h.pivot[0], h.pivot[1], h.pivot[2], 0); pivB[p] = make_float4(h.pivot[3], h.pivot[4], h.pivot[5], 0);
        axA[p] = pA[p] = qA[p] = axB[p] = pB[p] = make_float4(0, 0, 0, 0);
        if (h.type == EDYNHIP_JOINT_HINGE) {   // hinge_constraint::set_axes, hinge_constraint.cpp:11-17
            float p3[3], q3[3];
            plane_space_h(h.axis, p3, q3);
            axA[p] = make_float4(h.axis[0], h.axis[1], h.axis[2], 0); pA[p] = make_float4(p3[0], p3[1], p3[2], 0); qA[p] = make_float4(q3[0], q3[1], q3[2], 0);
            plane_space_h(h.axis + 3, p3, q3);
            axB[p] = make_float4(h.axis[3], h.axis[4], h.axis[5], 0); pB[p] = make_float4(p3[0], p3[1], p3[2], 0);
        } else if (h.has_frames) {   // cone / cvjoint / generic (the types that carry frames, append_host_joints): column k of a row-major 3x3 = elements k, 3 + k, 6 + k
            auto col = [&](int f, int k) { return make_float4(h.frame[9 * f + k], h.frame[9 * f + 3 + k], h.frame[9 * f + 6 + k], 0); };
            axA[p] = col(0, 0); pA[p] = col(0, 1); qA[p] = col(0, 2); axB[p] = col(1, 0); pB[p] = col(1, 1);
        }
        rows += joint_row_count(h.type);
        for (int k = 0; k < kJointParams; ++k) params[(size_t)k * j.cap + p] = h.params[k];
        for (int r = 0; r < kJointSlots; ++r) impulse[(size_t)r * j.cap + p] = h.impulse[r];
        angle[p] = h.angle;
    }
    j.num_colours = ncol; j.rows = rows;
    EH_HIP(c, hipMemcpyAsync(j.orig, orig.data(), n * 4, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.type, type.data(), n * 4, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.bodyA, bA.data(), n * 4, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.bodyB, bB.data(), n * 4, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.pivA, pivA.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.pivB, pivB.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.axA, axA.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.pA, pA.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.qA, qA.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.axB, axB.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.pB, pB.data(), n * 16, hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.params, params.data(), params.size() * sizeof(float), hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.impulse, impulse.data(), impulse.size() * sizeof(float), hipMemcpyHostToDevice, s));
    EH_HIP(c, hipMemcpyAsync(j.angle, angle.data(), n * sizeof(float), hipMemcpyHostToDevice, s));
    EH_HIP(c, hipStreamSynchronize(s));
    c->stats.num_joints = n; c->stats.num_joint_rows = rows; c->stats.num_joint_colours = ncol;
    return EDYNHIP_OK;
}
static int append_host_joints(edynhip_ctx *c, uint32_t n, const edynhip_joints *in, const char *who) {
    for (uint32_t e = 0; e < n; ++e) {
        HostJoint h;
        h.type = in->type[e]; h.body[0] = in->body[2 * e]; h.body[1] = in->body[2 * e + 1];
        if (h.body[0] >= c->b.n || h.body[1] >= c->b.n) return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": body index out of range").c_str());
        if (h.type < EDYNHIP_JOINT_POINT || h.type > EDYNHIP_JOINT_NULL) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, (std::string(who) + ": joint type").c_str());
        std::memcpy(h.pivot, in->pivot + 6 * e, sizeof(h.pivot));
        if (h.type == EDYNHIP_JOINT_HINGE) {
            if (!in->axis) return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": hinge needs axes").c_str());
            std::memcpy(h.axis, in->axis + 6 * e, sizeof(h.axis));
        }
        if (in->params) std::memcpy(h.params, in->params + (size_t)kJointApiParams * e, sizeof(float) * kJointApiParams);
        if (h.type == EDYNHIP_JOINT_CONE || h.type == EDYNHIP_JOINT_CVJOINT || h.type == EDYNHIP_JOINT_GENERIC) {   // identity frames, an open cone / free dofs, until defined
            const float id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            std::memcpy(h.frame, id, sizeof(id)); std::memcpy(h.frame + 9, id, sizeof(id));
            h.has_frames = true;
            if (h.type == EDYNHIP_JOINT_CONE && !(h.params[0] > 0 && h.params[1] > 0)) { h.params[0] = 1; h.params[1] = 1; }
        }
        c->host_joints.push_back(h);
    }
    return EDYNHIP_OK;
}
// reset_angle of the marked joints (sorted order) against the current pose
static int reset_marked_angles(edynhip_ctx *c, const std::vector<uint8_t> &which) {
    DeviceBuf<uint8_t> d;
    EH_HIP(c, d.alloc(which.size()));
    EH_HIP(c, hipMemcpyAsync(d, which.data(), which.size(), hipMemcpyHostToDevice, c->stream));
    int rc = joint_reset_angles(c, d);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}
// hinges whose parameters enable the angle-dependent rows start from the angle of the current pose (reset_angle)
static int reset_new_angles(edynhip_ctx *c, uint32_t first_caller_index) {
    Joints &j = c->j;
    if (j.n == 0) return EDYNHIP_OK;
    std::vector<uint32_t> orig(j.n);
    EH_HIP(c, hipMemcpyAsync(orig.data(), j.orig, (size_t)j.n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> which(j.n, 0);
    bool any = false;
    for (uint32_t p = 0; p < j.n; ++p) if (orig[p] >= first_caller_index) { which[p] = 1; any = true; }
    if (!any) return EDYNHIP_OK;
    return reset_marked_angles(c, which);
}
// Redefinitions are applied lazily: the host copy is edited at once, the device arrays are rebuilt (and the angles of the
// edited joints reset against the current orientations, as hinge_constraint / cvjoint_constraint::reset_angle) by the next entry
// point that reads or advances them - a figure's thousands of definitions cost one rebuild, not one each.
static int redefine_joint(edynhip_ctx *c, uint32_t joint, const float *params, int nparams, const float *frameA, const float *frameB) {
    std::memcpy(c->host_joints[joint].params, params, sizeof(float) * nparams);
    if (frameA) { std::memcpy(c->host_joints[joint].frame, frameA, 9 * sizeof(float)); std::memcpy(c->host_joints[joint].frame + 9, frameB, 9 * sizeof(float)); c->host_joints[joint].has_frames = true; }
    c->pending_redefs.push_back(joint);
    return EDYNHIP_OK;
}
int flush_joint_redefs(edynhip_ctx *c) {
    if (c->pending_redefs.empty()) return EDYNHIP_OK;
    std::vector<uint32_t> pending;
    pending.swap(c->pending_redefs);
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(rebuild_joints(c, true));    // applied impulses and angles of the others come from the device
    EH_TRY(rebuild_joints(c, false));
    if (c->j.n == 0) return EDYNHIP_OK;
    std::vector<uint8_t> edited(c->host_joints.size(), 0);
    for (uint32_t j : pending) if (j < edited.size()) edited[j] = 1;
    std::vector<uint32_t> orig(c->j.n);
    EH_HIP(c, hipMemcpyAsync(orig.data(), c->j.orig, (size_t)c->j.n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> which(c->j.n, 0);
    for (uint32_t p = 0; p < c->j.n; ++p) which[p] = edited[orig[p]];
    return reset_marked_angles(c, which);
}

// ---- collision exclusion lists (util/exclude_collision.cpp:9-71; the list itself: ctx_rules.hpp excl_*)
// The host list is edited at once; the device rows follow lazily, with the next entry point that runs the broadphase (flush_exclusions):
// a figure's 21 exclusions per rag doll - 21 504 calls for a field of 1 024 - cost one upload, not two 64-byte copies and a stream
// synchronisation each (43 042 copy launches at scene set-up).
static int upload_exclusion_rows(edynhip_ctx *c, uint32_t a, uint32_t b) {
    ExclusionLists &x = c->exclusions;
    x.dirty_lo = std::min(x.dirty_lo, std::min(a, b));
    x.dirty_hi = std::max(x.dirty_hi, std::max(a, b) + 1u);
    return EDYNHIP_OK;
}
int flush_exclusions(edynhip_ctx *c) {
    ExclusionLists &x = c->exclusions;
    if (x.dirty_lo >= x.dirty_hi) return EDYNHIP_OK;
    const uint32_t lo = x.dirty_lo, hi = std::min(x.dirty_hi, c->b.cap);
    x.dirty_lo = 0xFFFFFFFFu; x.dirty_hi = 0;
    if (x.host.empty() || lo >= hi) return EDYNHIP_OK;
    if (!c->excl) {
        EH_TRY(dalloc(c, c->excl, (size_t)c->b.cap * 16));
        EH_HIP(c, hipMemsetAsync(c->excl, 0xFF, (size_t)c->b.cap * 16 * sizeof(uint32_t), c->stream));
    }
    EH_HIP(c, hipMemcpyAsync(c->excl + (size_t)lo * 16, x.host.data() + (size_t)lo * 16, (size_t)(hi - lo) * 16 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));   // (the host list may be edited again right away)
    return EDYNHIP_OK;
}

}  // namespace eh

using namespace eh;

extern "C" {

int edynhip_set_bodies(edynhip_ctx *c, uint32_t n, const edynhip_bodies *in) { return load_bodies(c, 0, n, in, "edynhip_set_bodies"); }

int edynhip_add_bodies(edynhip_ctx *c, uint32_t n, const edynhip_bodies *in) {
    if (!c) return EDYNHIP_ERR_INVALID;
    return load_bodies(c, c->b.n, n, in, "edynhip_add_bodies");
}

// The island entity outlives a node it loses, and with it its sleep timer (island_manager.cpp:74-97, 421-424). Here an island is named by its
// lowest body index: where that body was removed, the name and the timer kept under it move to the lowest index that is left, so that the
// next relabel finds last step's island under a body that still exists - whole (the timer goes on) or split (k_cc_flatten restarts it).
// On the host: a removal synchronises anyway, and only worlds with island sleeping pay the two copies.
static int rename_islands_of_removed_roots(edynhip_ctx *c, const std::vector<uint8_t> &gone) {
    const uint32_t n = c->b.n;
    if (!c->sleeping || !c->island_labels_valid || n == 0) return EDYNHIP_OK;
    std::vector<uint32_t> label(n);
    std::vector<double> since(n);
    EH_HIP(c, hipMemcpyAsync(label.data(), c->b.island, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipMemcpyAsync(since.data(), c->sleep_since, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> heir(n, 0xFFFFFFFFu);
    bool changed = false;
    for (uint32_t i = 0; i < n; ++i) {   // ascending: the first member met is the lowest index left
        const uint32_t l = label[i];
        if (l >= n || l == i || !gone[l] || gone[i]) continue;
        if (heir[l] == 0xFFFFFFFFu) { heir[l] = i; since[i] = since[l]; }
        label[i] = heir[l];
        changed = true;
    }
    for (uint32_t i = 0; i < n; ++i) if (gone[i] && since[i] >= 0.0) { since[i] = -1.0; changed = true; }
    if (!changed) return EDYNHIP_OK;
    EH_HIP(c, hipMemcpyAsync(c->b.island, label.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipMemcpyAsync(c->sleep_since, since.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));   // the vectors go out of scope
    return EDYNHIP_OK;
}

int edynhip_remove_bodies(edynhip_ctx *c, uint32_t n, const uint32_t *indices) {
    if (!c || (n && !indices)) return EDYNHIP_ERR_INVALID;
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= c->b.n) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_remove_bodies: index out of range");
    // joints attached to a removed body go with it (the node's edges are destroyed, island_manager.cpp:56-62)
    std::vector<uint8_t> gone(c->b.n, 0);
    for (uint32_t k = 0; k < n; ++k) gone[indices[k]] = 1;
    bool joints_changed = false;
    std::vector<uint32_t> partners;
    if (!c->host_joints.empty()) {
        EH_TRY(flush_joint_redefs(c));
        EH_TRY(rebuild_joints(c, true));
        for (HostJoint &h : c->host_joints)
            if (h.alive && (gone[h.body[0]] || gone[h.body[1]])) { h.alive = false; joints_changed = true; partners.push_back(h.body[0]); partners.push_back(h.body[1]); }
    }
    uint32_t *list = nullptr;
    EH_TRY(index_scratch(c, n, list));
    EH_HIP(c, hipMemcpyAsync(list, indices, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipMemsetAsync(c->sleep_action, 0, (size_t)c->b.n * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_mark_removed, dim3(blocks(n, 128)), dim3(128), 0, c->stream, n, list, c->b, c->sleep_action);
    if (c->num_manifolds) hipLaunchKernelGGL(k_wake_partners, dim3(blocks(c->num_manifolds, 256)), dim3(256), 0, c->stream, c->num_manifolds, c->m[c->cur], c->b, c->sleep_action);
    hipLaunchKernelGGL(k_wake_marked, dim3(blocks(c->b.n, 256)), dim3(256), 0, c->stream, c->b.n, c->b, c->sleep_action, c->sleep_since, false);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_error(c, EDYNHIP_ERR_HIP, "edynhip_remove_bodies", e);
    EH_TRY(rename_islands_of_removed_roots(c, gone));
    for (uint32_t k = 0; k < n; ++k) { c->host_kind[indices[k]] = EDYNHIP_KIND_STATIC; c->host_shape[indices[k]] = EDYNHIP_SHAPE_NONE; c->host_removed[indices[k]] = 1; }
    std::vector<uint32_t> &excl = c->exclusions.host;
    if (!excl.empty())
        for (uint32_t k = 0; k < n; ++k) std::fill(excl.begin() + (size_t)indices[k] * 16, excl.begin() + (size_t)indices[k] * 16 + 16, 0xFFFFFFFFu);
    EH_TRY(rebuild_broadphase_lists(c));
    if (joints_changed) { EH_TRY(rebuild_joints(c, false)); EH_TRY(wake_islands_of(c, partners)); }
    invalidate_contact_state_replaced(c);
    return EDYNHIP_OK;
}

int edynhip_set_joints(edynhip_ctx *c, uint32_t n, const edynhip_joints *in) {
    if (!c || (n && !in)) return EDYNHIP_ERR_INVALID;
    if (n > c->j.cap) return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_set_joints: n > max_joints");
    EH_HIP(c, hipSetDevice(c->device));
    c->host_joints.clear();
    c->pending_redefs.clear();
    c->sleep_prev_joints = 0;   // the caller indices start again: none of the new joints is an edge of last step's islands
    if (n) EH_TRY(append_host_joints(c, n, in, "edynhip_set_joints"));
    EH_TRY(rebuild_joints(c, false));
    return reset_new_angles(c, 0);
}
int edynhip_add_joints(edynhip_ctx *c, uint32_t n, const edynhip_joints *in, uint32_t *first_index) {
    if (!c || (n && !in)) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    const uint32_t first = (uint32_t)c->host_joints.size();
    if (first_index) *first_index = first;
    if (n == 0) return EDYNHIP_OK;
    EH_TRY(flush_joint_redefs(c));
    EH_TRY(append_host_joints(c, n, in, "edynhip_add_joints"));
    int rc = rebuild_joints(c, true);
    if (rc != EDYNHIP_OK) { c->host_joints.resize(first); (void)rebuild_joints(c, false); return rc; }
    EH_TRY(reset_new_angles(c, first));
    // a new edge wakes the islands it joins (insert_to_island, island_manager.cpp:282-294)
    std::vector<uint32_t> ends;
    for (size_t k = first; k < c->host_joints.size(); ++k) { ends.push_back(c->host_joints[k].body[0]); ends.push_back(c->host_joints[k].body[1]); }
    return wake_islands_of(c, ends);
}
int edynhip_remove_joints(edynhip_ctx *c, uint32_t n, const uint32_t *indices) {
    if (!c || (n && !indices)) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= c->host_joints.size()) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_remove_joints: index out of range");
    EH_TRY(flush_joint_redefs(c));
    // fetch first: the impulses of the survivors come from the device
    EH_TRY(rebuild_joints(c, true));
    std::vector<uint32_t> touched;
    for (uint32_t k = 0; k < n; ++k) {
        HostJoint &h = c->host_joints[indices[k]];
        if (!h.alive) continue;
        h.alive = false;
        touched.push_back(h.body[0]); touched.push_back(h.body[1]);
    }
    EH_TRY(rebuild_joints(c, false));
    return wake_islands_of(c, touched);   // destroying an edge wakes its island (island_manager.cpp:74-97)
}
int edynhip_set_joint_params(edynhip_ctx *c, uint32_t joint, const float *params) {
    if (!c || !params || joint >= c->host_joints.size() || !c->host_joints[joint].alive) return EDYNHIP_ERR_INVALID;
    return redefine_joint(c, joint, params, kJointApiParams, nullptr, nullptr);
}
int edynhip_set_joint_definition(edynhip_ctx *c, uint32_t joint, const float *frameA, const float *frameB, const float *params16) {
    if (!c || !params16 || !frameA || !frameB || joint >= c->host_joints.size() || !c->host_joints[joint].alive) return EDYNHIP_ERR_INVALID;
    const int t = c->host_joints[joint].type;
    if (t != EDYNHIP_JOINT_CONE && t != EDYNHIP_JOINT_CVJOINT) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_joint_definition: cone and cvjoint constraints only");
    if (t == EDYNHIP_JOINT_CONE && !(params16[0] > 0 && params16[1] > 0)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_joint_definition: cone span tangents must be positive");
    return redefine_joint(c, joint, params16, 16, frameA, frameB);
}
int edynhip_set_generic_definition(edynhip_ctx *c, uint32_t joint, const float *frameA, const float *frameB, const float *dof60) {
    if (!c || !dof60 || !frameA || !frameB || joint >= c->host_joints.size() || !c->host_joints[joint].alive) return EDYNHIP_ERR_INVALID;
    if (c->host_joints[joint].type != EDYNHIP_JOINT_GENERIC) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_generic_definition: generic constraints only");
    for (int d = 0; d < 6; ++d)
        if (dof60[10 * d] != 0 && dof60[10 * d + 1] > dof60[10 * d + 2]) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_generic_definition: a limit's minimum exceeds its maximum");
    return redefine_joint(c, joint, dof60, 60, frameA, frameB);
}
int edynhip_set_joint_warm_start(edynhip_ctx *c, const float *impulses24, const float *angles) {
    if (!c || !impulses24) return EDYNHIP_ERR_INVALID;
    const uint32_t total = (uint32_t)c->host_joints.size();
    if (total == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(flush_joint_redefs(c));
    for (uint32_t e = 0; e < total; ++e) {
        HostJoint &h = c->host_joints[e];
        if (!h.alive) continue;
        std::memcpy(h.impulse, impulses24 + (size_t)kJointSlots * e, sizeof(h.impulse));
        if (angles) h.angle = angles[e];
    }
    return rebuild_joints(c, false);   // host copies -> device (colouring unchanged: same joints)
}
int edynhip_get_joint_slot_impulses(edynhip_ctx *c, float *out) {
    if (!c || !out) return EDYNHIP_ERR_INVALID;
    const uint32_t total = (uint32_t)c->host_joints.size();
    if (total == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(flush_joint_redefs(c));
    std::memset(out, 0, (size_t)total * kJointSlots * sizeof(float));
    const uint32_t n = c->j.n;
    if (n == 0) return EDYNHIP_OK;
    std::vector<float> imp((size_t)c->j.cap * kJointSlots);
    std::vector<uint32_t> orig(n);
    EH_HIP(c, hipMemcpyAsync(imp.data(), c->j.impulse, imp.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipMemcpyAsync(orig.data(), c->j.orig, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t p = 0; p < n; ++p)
        for (int r = 0; r < kJointSlots; ++r) out[(size_t)kJointSlots * orig[p] + r] = imp[(size_t)r * c->j.cap + p];
    return EDYNHIP_OK;
}
int edynhip_get_joint_impulses(edynhip_ctx *c, float *out) {
    if (!c || !out) return EDYNHIP_ERR_INVALID;
    const uint32_t total = (uint32_t)c->host_joints.size();
    if (total == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    EH_TRY(flush_joint_redefs(c));
    std::memset(out, 0, (size_t)total * 10 * sizeof(float));
    const uint32_t n = c->j.n;
    if (n == 0) return EDYNHIP_OK;
    std::vector<float> imp((size_t)c->j.cap * kJointSlots), ang(n);
    std::vector<uint32_t> orig(n);
    EH_HIP(c, hipMemcpyAsync(imp.data(), c->j.impulse, imp.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipMemcpyAsync(ang.data(), c->j.angle, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipMemcpyAsync(orig.data(), c->j.orig, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t p = 0; p < n; ++p) {
        for (int r = 0; r < kJointApiSlots; ++r) out[10 * (size_t)orig[p] + r] = imp[(size_t)r * c->j.cap + p];
        out[10 * (size_t)orig[p] + 9] = ang[p];
    }
    return EDYNHIP_OK;
}

// ---- sleep and wake edits
__global__ void k_set_asleep(uint32_t n, Bodies b, const uint8_t *__restrict__ asleep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t fl = b.flags[i];
    if ((fl & BF_KIND_MASK) != EDYNHIP_KIND_DYNAMIC || (fl & (BF_REMOVED | BF_NOSLEEP))) return;
    if (asleep[i]) {   // put_to_sleep (island_manager.cpp:553-565): tag + zero velocities
        b.flags[i] = fl | BF_ASLEEP;
        b.linvel[i] = make_float4(0, 0, 0, 0); b.angvel[i] = make_float4(0, 0, 0, 0);
    } else b.flags[i] = fl & ~BF_ASLEEP;
}
int edynhip_set_asleep(edynhip_ctx *c, const uint8_t *asleep) {
    if (!c || !asleep) return EDYNHIP_ERR_INVALID;
    if (!c->sleeping || c->b.n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    uint32_t *buf = nullptr;
    EH_TRY(index_scratch(c, (c->b.n + 3) / 4, buf));
    EH_HIP(c, hipMemcpyAsync(buf, asleep, c->b.n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_set_asleep, dim3(blocks(c->b.n, 256)), dim3(256), 0, c->stream, c->b.n, c->b, (const uint8_t *)buf);
    EH_HIP(c, hipStreamSynchronize(c->stream));
    invalidate_graph_changed(c, true);   // asleep or not is decided again by the next step
    return EDYNHIP_OK;
}
int edynhip_get_sleep_timers(edynhip_ctx *c, uint32_t *island_label, double *since, double *clock) {
    if (!c || !island_label || !since || !clock) return EDYNHIP_ERR_INVALID;
    *clock = c->sim_clock;
    const uint32_t n = c->b.n;
    if (n == 0) return EDYNHIP_OK;
    // no island stage has run yet on this scene (a re-partition before the first step): every body is its own island, no timer runs
    if (!c->sleeping || !c->island_labels_valid) { for (uint32_t i = 0; i < n; ++i) { island_label[i] = i; since[i] = -1.0; } return EDYNHIP_OK; }
    EH_HIP(c, hipSetDevice(c->device));
    EH_HIP(c, hipMemcpyAsync(island_label, c->b.island, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipMemcpyAsync(since, c->sleep_since, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    return EDYNHIP_OK;
}
int edynhip_set_sleep_timers(edynhip_ctx *c, const uint32_t *island_label, const double *since, double clock) {
    if (!c || !island_label || !since) return EDYNHIP_ERR_INVALID;
    const uint32_t n = c->b.n;
    if (!c->sleeping || n == 0) return EDYNHIP_OK;
    for (uint32_t i = 0; i < n; ++i) if (island_label[i] >= n) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_sleep_timers: island label out of range");
    EH_HIP(c, hipSetDevice(c->device));
    // The labels become "last step's labels": the next step's relabel (forced below) starts from them, so its merge / split rules
    // (k_sleep_sizes / k_sleep_carry, k_cc_flatten's split marks) see the islands the timers belong to.
    EH_HIP(c, hipMemcpyAsync(c->b.island, island_label, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipMemcpyAsync(c->sleep_since, since, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    c->sim_clock = clock;
    c->sleep_prev_n = n;
    c->sleep_prev_joints = (uint32_t)c->host_joints.size();   // the joints came with the state: edges of the islands the timers belong to
    invalidate_graph_changed(c, false);
    c->island_labels_valid = true;
    return EDYNHIP_OK;
}
__global__ void k_wake_all(uint32_t n, uint32_t *flags, double *since) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] &= ~BF_ASLEEP;
    since[i] = -1.0;
}
int edynhip_wake_all(edynhip_ctx *c) {
    if (!c) return EDYNHIP_ERR_INVALID;
    invalidate_woke(c);
    if (c->b.n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_wake_all, dim3(blocks(c->b.n, 256)), dim3(256), 0, c->stream, c->b.n, c->b.flags, c->sleep_since);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}
int edynhip_wake_bodies(edynhip_ctx *c, uint32_t n, const uint32_t *indices) {
    if (!c || (n && !indices)) return EDYNHIP_ERR_INVALID;
    for (uint32_t k = 0; k < n; ++k) if (indices[k] >= c->b.n) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_wake_bodies: index out of range");
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    return wake_islands_of(c, std::vector<uint32_t>(indices, indices + n));
}

// ---- parameters and gravity
int edynhip_get_params(edynhip_ctx *c, edynhip_params *out) {
    if (!c || !out) return EDYNHIP_ERR_INVALID;
    out->fixed_dt = c->cfg.fixed_dt;
    out->num_velocity_iterations = c->cfg.num_velocity_iterations;
    out->num_position_iterations = c->cfg.num_position_iterations;
    std::memcpy(out->gravity, c->cfg.gravity, sizeof(out->gravity));
    out->num_restitution_iterations = c->restitution_iterations;
    out->num_individual_restitution_iterations = c->individual_restitution_iterations;
    return EDYNHIP_OK;
}
__global__ void k_set_gravity(uint32_t n, Bodies b, float4 g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (b.flags[i] & BF_KIND_MASK) == EDYNHIP_KIND_DYNAMIC) b.grav[i] = g;
}
int edynhip_set_params(edynhip_ctx *c, const edynhip_params *p) {
    if (!c || !p || !(p->fixed_dt > 0)) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    c->cfg.fixed_dt = p->fixed_dt;
    c->cfg.num_velocity_iterations = p->num_velocity_iterations;
    c->cfg.num_position_iterations = p->num_position_iterations;
    c->restitution_iterations = p->num_restitution_iterations;
    c->individual_restitution_iterations = p->num_individual_restitution_iterations;
    if (std::memcmp(c->cfg.gravity, p->gravity, sizeof(p->gravity)) != 0) {   // set_gravity: the setting and every body's gravity
        std::memcpy(c->cfg.gravity, p->gravity, sizeof(p->gravity));
        if (c->b.n) hipLaunchKernelGGL(k_set_gravity, dim3(blocks(c->b.n, 256)), dim3(256), 0, c->stream, c->b.n, c->b, make_float4(p->gravity[0], p->gravity[1], p->gravity[2], 0));
        EH_HIP(c, hipGetLastError());
        if (c->sleeping) EH_TRY(edynhip_wake_all(c));
    }
    return EDYNHIP_OK;
}

// ---- centre of mass
__global__ void k_move_com(Bodies b, uint32_t i, float3 com_new) {
    const f3 com = mk3(com_new.x, com_new.y, com_new.z);
    const float4 p4 = B_POS(b, i);
    const f3 pos = from4(p4);
    const q4 orn = q_from4(B_ORN(b, i));
    const f3 origin = b.com[i].w != 0.0f ? to_world(-from4(b.com[i]), pos, orn) : pos;
    const f3 com_world = to_world(com, origin, orn);
    if ((b.flags[i] & BF_KIND_MASK) != EDYNHIP_KIND_STATIC) b.linvel[i] = to4(from4(b.linvel[i]) + cross(from4(b.angvel[i]), com_world - pos), 0);
    B_POS(b, i) = to4(com_world, p4.w);
    const bool has = !(com.x == 0 && com.y == 0 && com.z == 0);
    b.com[i] = to4(has ? com : mk3(0, 0, 0), has ? 1.0f : 0.0f);
    b.origin[i] = to4(origin, 0);
}
int edynhip_set_center_of_mass(edynhip_ctx *c, uint32_t body, const float *com3) {
    if (!c || !com3 || body >= c->b.n) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    if (!c->b.com) {   // the first offset of this world: attach the (zeroed) origin arrays
        EH_HIP(c, hipMemsetAsync(c->com_store, 0, (size_t)c->b.cap * sizeof(float4), c->stream));
        c->b.com = c->com_store; c->b.origin = c->origin_store;
    }
    hipLaunchKernelGGL(k_move_com, dim3(1), dim3(1), 0, c->stream, c->b, body, make_float3(com3[0], com3[1], com3[2]));
    EH_HIP(c, hipGetLastError());
    invalidate_bodies_moved(c);   // (the reference does not wake the body's island either)
    return EDYNHIP_OK;
}

// ---- exclusions and the pair filter
int edynhip_exclude_collision(edynhip_ctx *c, uint32_t a, uint32_t b) {
    if (!c || a >= c->b.n || b >= c->b.n || a == b) return EDYNHIP_ERR_INVALID;
    EH_HIP(c, hipSetDevice(c->device));
    std::vector<uint32_t> &l = c->exclusions.host;
    if (l.empty()) l.assign((size_t)c->b.cap * 16, 0xFFFFFFFFu);
    if (!excl_add(&l[(size_t)a * 16], b) || !excl_add(&l[(size_t)b * 16], a))
        return set_error(c, EDYNHIP_ERR_CAPACITY, "edynhip_exclude_collision: more than 16 exclusions on one body (collision_exclusion::max_exclusions)");
    return upload_exclusion_rows(c, a, b);
}
int edynhip_remove_collision_exclusion(edynhip_ctx *c, uint32_t a, uint32_t b) {
    if (!c || a >= c->b.n || b >= c->b.n) return EDYNHIP_ERR_INVALID;
    std::vector<uint32_t> &l = c->exclusions.host;
    if (l.empty()) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    excl_drop(&l[(size_t)a * 16], b); excl_drop(&l[(size_t)b * 16], a);
    return upload_exclusion_rows(c, a, b);
}
int edynhip_set_pair_filter(edynhip_ctx *c, edynhip_pair_filter filter, void *user) {
    if (!c) return EDYNHIP_ERR_INVALID;
    c->pair_filter = filter; c->pair_filter_user = user;
    if (filter && !c->filter_new_idx) {
        EH_HIP(c, hipSetDevice(c->device));
        EH_TRY(dalloc(c, c->filter_new_idx, c->cfg.max_manifolds));
    }
    return EDYNHIP_OK;
}
int edynhip_default_should_collide(edynhip_ctx *c, uint32_t a, uint32_t b) {   // should_collide_default, should_collide.cpp:11-57
    if (!c || a >= c->b.n || b >= c->b.n) return EDYNHIP_ERR_INVALID;
    return should_collide_default(a, b, c->host_group, c->host_mask, c->exclusions.host);
}

}  // extern "C"

// ---- contact_extras materials (comp/material.hpp:15-22; contact_extras_constraint.cpp)
namespace eh {
static int ensure_extras_storage(edynhip_ctx *c) {   // the per-point storage and the extras rows come into existence with the first such material
    if (!c->m[0].xmat) {
        for (int k = 0; k < 2; ++k) {
            EH_TRY(dalloc(c, c->m[k].xmat, (size_t)c->m[k].cap * kMaxPts)); EH_TRY(dalloc(c, c->m[k].ximp, (size_t)c->m[k].cap * kMaxPts));
        }
        EH_TRY(dalloc(c, c->rows.rwx, (size_t)c->m[0].cap * kMaxPts * kXPoint));
        // points that already exist keep plain contact_constraint behaviour: default material, no impulses
        std::vector<float4> def((size_t)c->m[0].cap * kMaxPts, make_float4(0, 0, kLarge, kLarge));
        for (int k = 0; k < 2; ++k) EH_HIP(c, hipMemcpyAsync(c->m[k].xmat, def.data(), def.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        EH_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->extras = true;
    return EDYNHIP_OK;
}
// ---- material ids and the mix table (material_mixing.hpp:36-82, util/insert_material_mixing.cpp)
static int rebuild_mix_table(edynhip_ctx *c) {
    MixTable &mx = c->mix;
    const uint32_t nb = c->b.n;
    mx.mat_id.resize(nb, 0xFFFFu);
    std::map<uint32_t, uint32_t> compact;   // material id -> compact index, ids in use only
    for (uint32_t i = 0; i < nb; ++i) if (mx.mat_id[i] != 0xFFFFu) compact.emplace(mx.mat_id[i], 0u);
    uint32_t K = 0;
    for (auto &kv : compact) kv.second = K++;
    if (mx.host.empty() || K == 0) { c->b.mix_K = 0; return EDYNHIP_OK; }
    std::vector<uint32_t> cid(nb, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < nb; ++i) if (mx.mat_id[i] != 0xFFFFu) cid[i] = compact[mx.mat_id[i]];
    std::vector<float> vals;
    std::map<const void *, int32_t> entry_index;
    bool extras = false;
    for (auto &kv : mx.host) {
        entry_index[&kv.second] = (int32_t)(vals.size() / 6);
        vals.insert(vals.end(), kv.second.begin(), kv.second.end());
        if (kv.second[0] > 0) c->has_restitution = true;
        extras = extras || kv.second[2] > 0 || kv.second[3] > 0 || kv.second[4] < kLarge || kv.second[5] < kLarge;
    }
    std::vector<int32_t> lut((size_t)K * K, -1);
    for (auto &a : compact)
        for (auto &b : compact) {   // the reference's own lookup, ordered pair (id of body[0], id of body[1])
            auto it = mx.host.find(MixIdPair{a.first, b.first});
            if (it != mx.host.end()) lut[(size_t)a.second * K + b.second] = entry_index[&it->second];
        }
    if (extras) EH_TRY(ensure_extras_storage(c));
    if (!mx.d_mat_cid) EH_TRY(dalloc(c, mx.d_mat_cid, c->b.cap));
    if (mx.lut_cap < lut.size()) { mx.d_lut = nullptr; EH_TRY(dalloc(c, mx.d_lut, lut.size())); mx.lut_cap = (uint32_t)lut.size(); }
    if (mx.vals_cap < vals.size()) { mx.d_vals = nullptr; EH_TRY(dalloc(c, mx.d_vals, vals.size())); mx.vals_cap = (uint32_t)vals.size(); }
    EH_HIP(c, hipMemcpyAsync(mx.d_mat_cid, cid.data(), (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipMemcpyAsync(mx.d_lut, lut.data(), lut.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipMemcpyAsync(mx.d_vals, vals.data(), vals.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    c->b.mat_cid = mx.d_mat_cid; c->b.mix_lut = mx.d_lut; c->b.mix_vals = mx.d_vals; c->b.mix_K = K;
    return EDYNHIP_OK;
}
}  // namespace eh

namespace eh {

int shard_set_material_extras(edynhip_ctx *c, uint32_t first, uint32_t n, const float *spin, const float *roll, const float *stiffness, const float *damping) {
    if (!c) return EDYNHIP_ERR_INVALID;
    if ((uint64_t)first + n > c->b.n) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_material_extras: body range out of bounds");
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    std::vector<float4> h(n);
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        h[i] = make_float4(spin ? spin[i] : 0.0f, roll ? roll[i] : 0.0f, stiffness ? stiffness[i] : kLarge, damping ? damping[i] : kLarge);
        if (h[i].x < 0 || h[i].y < 0 || !(h[i].z > 0) || !(h[i].w > 0)) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_material_extras: negative friction or non-positive stiffness / damping");
        any = any || h[i].x > 0 || h[i].y > 0 || h[i].z < kLarge || h[i].w < kLarge;
    }
    if (any) EH_TRY(ensure_extras_storage(c));
    EH_HIP(c, hipMemcpyAsync(c->b.mat2 + first, h.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    EH_HIP(c, hipStreamSynchronize(c->stream));
    return EDYNHIP_OK;
}
int shard_set_material_ids(edynhip_ctx *c, uint32_t first, uint32_t n, const uint32_t *ids) {
    if (!c || (n && !ids)) return EDYNHIP_ERR_INVALID;
    if ((uint64_t)first + n > c->b.n) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_material_ids: body range out of bounds");
    for (uint32_t i = 0; i < n; ++i) if (ids[i] > 0xFFFFu) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_set_material_ids: material::id_type is 16 bits (0xFFFF = unassigned)");
    EH_HIP(c, hipSetDevice(c->device));
    c->mix.mat_id.resize(c->b.n, 0xFFFFu);
    for (uint32_t i = 0; i < n; ++i) c->mix.mat_id[first + i] = ids[i];
    return rebuild_mix_table(c);
}
int shard_insert_material_mixing(edynhip_ctx *c, uint32_t id0, uint32_t id1, const float *material6) {
    if (!c || !material6) return EDYNHIP_ERR_INVALID;
    if (id0 >= 0xFFFFu || id1 >= 0xFFFFu) return set_error(c, EDYNHIP_ERR_INVALID, "edynhip_insert_material_mixing: unassigned material id");
    EH_HIP(c, hipSetDevice(c->device));
    c->mix.host[MixIdPair{id0, id1}] = {material6[0], material6[1], material6[2], material6[3], material6[4], material6[5]};
    return rebuild_mix_table(c);
}
// An empty mix table, before the bodies of a (re)built shard go up: the world replays its insertions, in their order, afterwards. The table is the reference's
// std::map under unordered_pair's comparator, which is no strict weak order - inserting (1, 0) into a table that holds only (0, 1)
// overwrites that entry, into one that also holds (0, 2) and (1, 2) it makes a new one - so a replay on top of what a kept context
// still holds would build another table than the one context that took the same insertions once.
int shard_reset_material_mixing(edynhip_ctx *c) {
    c->mix.host.clear();
    c->b.mix_K = 0;
    return EDYNHIP_OK;
}
int shard_ensure_extras_storage(edynhip_ctx *c) {
    EH_HIP(c, hipSetDevice(c->device));
    return ensure_extras_storage(c);
}

}  // namespace eh

extern "C" {

// (a shard of a multi-device world holds part of the world's bodies in local indices: its materials are the world's, edynhip_world_set_material_extras ...)
static int refuse_shard(edynhip_ctx *c, const char *who) {
    return set_error(c, EDYNHIP_ERR_UNSUPPORTED, (std::string(who) + ": a shard of a multi-device world takes its materials from the world").c_str());
}
int edynhip_set_material_extras(edynhip_ctx *c, uint32_t first, uint32_t n, const float *spin, const float *roll, const float *stiffness, const float *damping) {
    if (c && c->world_shard) return refuse_shard(c, "edynhip_set_material_extras");
    return shard_set_material_extras(c, first, n, spin, roll, stiffness, damping);
}
int edynhip_set_material_ids(edynhip_ctx *c, uint32_t first, uint32_t n, const uint32_t *ids) {
    if (c && c->world_shard) return refuse_shard(c, "edynhip_set_material_ids");
    return shard_set_material_ids(c, first, n, ids);
}
int edynhip_insert_material_mixing(edynhip_ctx *c, uint32_t id0, uint32_t id1, const float *material6) {
    if (c && c->world_shard) return refuse_shard(c, "edynhip_insert_material_mixing");
    return shard_insert_material_mixing(c, id0, id1, material6);
}

}  // extern "C"
