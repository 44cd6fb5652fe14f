// Raycast queries (edyn::raycast, src/edyn/collision/raycast.cpp:20-56) for batches of rays, answered on the device.
// The reference walks its broadphase trees with the segment, tests every leaf whose fat AABB (the AABB grown by 0.1,
// dynamic_tree.hpp:24) the segment crosses (intersect_segment_aabb) with shape_raycast, and keeps the smallest fraction.
// Here the query tree is the context's own linear BVH over every shaped non-plane body (Morton keys, Karras build and ropes
// by the broadphase's kernels, on buffers of its own - broadphase.hip build_query_tree), rebuilt at the first raycast after
// anything changed the state (edynhip_ctx::state_epoch); planes, whose boxes are the huge half-space boxes, are a short list
// that every ray tests. One lane per ray walks the tree stackless along the ropes.
//   Leaves hold exactly the candidate predicate's box (AABB - 0.1, AABB + 0.1) and run exactly its test, so which bodies are
// tested does not depend on the tree. Internal nodes run the same segment-box test on the union of their children grown by
// kNodeGrow x (1 + |largest coordinate|), against a box grown further by the same relative amount of the ray's coordinates: the
// test is monotone in the box (a box that contains another passes every segment the smaller one passes), and the growth is
// far beyond the few ulps by which the rounded test can differ from the exact one, so no subtree that holds a passing leaf is
// ever skipped. No pruning by the best fraction so far: box and plane fractions can be negative, every overlapping leaf is tested.
#include "ctx.hpp"
#include "dpolyhedron.hpp"
#include "draycast.hpp"
#include "raytree.hpp"
#include <algorithm>
#include <cstring>

namespace eh {
using namespace dm;

constexpr float kNodeGrow = 1e-5f;            // relative growth of internal node boxes and of the ray's tolerance (see above)
constexpr uint32_t kNoBody = 0xFFFFFFFFu;
constexpr uint32_t kChunk = 1u << 20;          // rays per launch (and per staging buffer of the host entry point)

void raycast_free(edynhip_ctx *c) {
    if (!c->ray) return;
    for (void *p : c->ray->allocs) (void)hipFree(p);
    delete c->ray;
    c->ray = nullptr;
}

template <typename T>
static int ralloc(edynhip_ctx *c, RayTree &t, T *&p, size_t count) {
    void *q = nullptr;
    EH_HIP(c, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    t.allocs.push_back(q);
    p = (T *)q;
    return EDYNHIP_OK;
}

// The shape frame (origin when the body has a centre-of-mass offset, raycast.cpp:31-34) and the AABB of every shaped body from its
// current transform, with the arithmetic of solver.hip derive_body (update_origins, update_aabbs): equal to what a step leaves in the
// context's arrays, and right also where edynhip_set_state left those stale. Planes keep their half-space box (capi.hip upload).
__global__ void k_rc_boxes(uint32_t n, Bodies b, dc::Meshes meshes, float4 *org, float4 *amin, float4 *amax) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t fl = b.flags[i];
    const int st = (int)((fl & BF_SHAPE_MASK) >> BF_SHAPE_SHIFT);
    if (st == dc::SHAPE_NONE) return;
    const q4 orn = q_from4(B_ORN(b, i));
    f3 pos = from4(B_POS(b, i));
    if (b.origin && b.com[i].w != 0.0f) pos = to_world(-from4(b.com[i]), pos, orn);
    org[i] = to4(pos, 0);
    if (st == dc::SHAPE_PLANE) { amin[i] = b.amin[i]; amax[i] = b.amax[i]; return; }
    const m3 basis = to_m3(orn);
    if (st == dc::SHAPE_BOX) {   // aabb_util.cpp:42-63
        const f3 h = from4(b.shape[i]);
        float mn[3] = {pos.x, pos.y, pos.z}, mx[3] = {pos.x, pos.y, pos.z};
        const f3 rws[3] = {basis.r0, basis.r1, basis.r2};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cidx = 0; cidx < 3; ++cidx) {
                float e = comp(rws[r], cidx) * -comp(h, cidx);
                float f = -e;
                if (e < f) { mn[r] += e; mx[r] += f; } else { mn[r] += f; mx[r] += e; }
            }
        amin[i] = make_float4(mn[0], mn[1], mn[2], 0);
        amax[i] = make_float4(mx[0], mx[1], mx[2], 0);
    } else if (st == dc::SHAPE_SPHERE) {   // aabb_util.cpp:65-70
        const float r = b.shape[i].x;
        amin[i] = make_float4(pos.x - r, pos.y - r, pos.z - r, 0);
        amax[i] = make_float4(pos.x + r, pos.y + r, pos.z + r, 0);
    } else if (st == dc::SHAPE_CAPSULE) {   // aabb_util.cpp:81-88
        const float4 sh = b.shape[i];
        const f3 v = rotate(orn, dc::axis_vector(sh.z)) * sh.y;
        const f3 p0 = pos - v, p1 = pos + v;
        amin[i] = make_float4(fminf(p0.x, p1.x) - sh.x, fminf(p0.y, p1.y) - sh.x, fminf(p0.z, p1.z) - sh.x, 0);
        amax[i] = make_float4(fmaxf(p0.x, p1.x) + sh.x, fmaxf(p0.y, p1.y) + sh.x, fmaxf(p0.z, p1.z) + sh.x, 0);
    } else if (st == dc::SHAPE_CYLINDER) {   // aabb_util.cpp:72-79
        const box3 bb = dc::cylinder_aabb(dc::cyl_of(b.shape[i]), pos, orn);
        amin[i] = to4(bb.mn, 0); amax[i] = to4(bb.mx, 0);
    } else if (st == dc::SHAPE_POLYHEDRON) {   // update_aabbs.cpp:22-32
        const box3 bb = dc::polyhedron_aabb(meshes, b.shape[i], pos, orn);
        amin[i] = to4(bb.mn, 0); amax[i] = to4(bb.mx, 0);
    }
}

DI f3 fat_min(float4 a) { return mk3(a.x - kFatInset, a.y - kFatInset, a.z - kFatInset); }   // aabb.inset(-0.1): min + (-0.1)
DI f3 fat_max(float4 a) { return mk3(a.x + kFatInset, a.y + kFatInset, a.z + kFatInset); }   //                  max - (-0.1)
DI float max_abs(f3 a, f3 b) { return fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(b.x))), fmaxf(fabsf(b.y), fabsf(b.z))); }

// Node boxes cross workgroups inside this launch: agent-scope atomics on both sides (as broadphase.hip k_bp_refit does).
DI void rc_store(float4 *nmin, float4 *nmax, uint32_t node, f3 mn, f3 mx, uint32_t w0, uint32_t w1) {
    unsigned long long *a = (unsigned long long *)&nmin[node], *b = (unsigned long long *)&nmax[node];
    auto pk = [](float x, float y) { return ((unsigned long long)__float_as_uint(y) << 32) | __float_as_uint(x); };
    __hip_atomic_store(a, pk(mn.x, mn.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a + 1, pk(mn.z, __uint_as_float(w0)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(b, pk(mx.x, mx.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(b + 1, pk(mx.z, __uint_as_float(w1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
DI void rc_load(const float4 *nmin, const float4 *nmax, uint32_t node, f3 &mn, f3 &mx) {
    unsigned long long *a = (unsigned long long *)&nmin[node], *b = (unsigned long long *)&nmax[node];
    const unsigned long long x0 = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long x1 = __hip_atomic_load(a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long y0 = __hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long y1 = __hip_atomic_load(b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mn = mk3(__uint_as_float((uint32_t)x0), __uint_as_float((uint32_t)(x0 >> 32)), __uint_as_float((uint32_t)x1));
    mx = mk3(__uint_as_float((uint32_t)y0), __uint_as_float((uint32_t)(y0 >> 32)), __uint_as_float((uint32_t)y1));
}

// Bottom-up refit: the second child to arrive at a node writes its box (k_bp_build zeroed the arrival counters).
__global__ void k_rc_refit(uint32_t n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ left,
                           const uint32_t *__restrict__ right, const uint32_t *__restrict__ rope, const float4 *__restrict__ amin,
                           const float4 *__restrict__ amax, float4 *nmin, float4 *nmax, uint32_t *visit) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t body = (uint32_t)(keys[k] & 0xFFFFFFFFu);
    uint32_t node = n - 1 + k;
    f3 mn = fat_min(amin[body]), mx = fat_max(amax[body]);
    rc_store(nmin, nmax, node, mn, mx, kLeafBit | body, rope[node]);
    uint32_t p = parent[node];
    while (p != 0xFFFFFFFFu) {
        const uint32_t old = __hip_atomic_fetch_add(&visit[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0) return;   // the first arriver leaves; the second one has both children's boxes
        const uint32_t sib = left[p] == node ? right[p] : left[p];
        f3 smn, smx;
        rc_load(nmin, nmax, sib, smn, smx);
        mn = mk3(fminf(mn.x, smn.x), fminf(mn.y, smn.y), fminf(mn.z, smn.z));
        mx = mk3(fmaxf(mx.x, smx.x), fmaxf(mx.y, smx.y), fmaxf(mx.z, smx.z));
        const float g = kNodeGrow * (1.0f + max_abs(mn, mx));
        mn = mn - mk3(g, g, g); mx = mx + mk3(g, g, g);
        rc_store(nmin, nmax, p, mn, mx, left[p], rope[p]);
        node = p;
        p = parent[p];
    }
}

struct RayArgs {
    const float4 *xf;                 // Bodies::xf (orientation at 8 i + 1)
    const uint32_t *flags;
    const float4 *shape, *org, *amin, *amax;
    dc::Meshes meshes;
    const float4 *nmin, *nmax;
    uint32_t n_tree;
    const uint32_t *planes;
    uint32_t n_planes;
    uint32_t n_bodies;
    const uint32_t *ignore;           // bit per body, or nullptr
    const uint32_t *answers;          // a shard of a multi-device world: bit per body it answers for; nullptr: every body
    uint32_t brute;
};

struct Best { dr::RayHit h; uint32_t body; };

// One candidate: the ignore list, the candidate predicate, shape_raycast, and the keep-the-smallest rule (raycast.cpp:37-40; an exact
// tie goes to the lower body index). kList: the ignore list is the ray's own (lst[len], body indices in any order, duplicates and
// indices beyond the body count allowed - the tickets of query_async.hip) instead of the call's bit mask.
template <bool kList>
DI void rc_candidate(const RayArgs &a, uint32_t body, f3 p0, f3 p1, Best &best, const uint32_t *lst, uint32_t len) {
    if (kList) {
        for (uint32_t k = 0; k < len; ++k)
            if (lst[k] == body) return;
    } else if (a.ignore && ((a.ignore[body >> 5] >> (body & 31u)) & 1u)) return;
    if (a.answers && !((a.answers[body >> 5] >> (body & 31u)) & 1u)) return;   // another shard's to answer
    const uint32_t fl = a.flags[body];
    const int st = (int)((fl & BF_SHAPE_MASK) >> BF_SHAPE_SHIFT);
    if (st == dc::SHAPE_NONE || (fl & BF_REMOVED)) return;
    if (!dr::intersect_segment_aabb(p0, p1, fat_min(a.amin[body]), fat_max(a.amax[body]))) return;
    const float4 sh = a.shape[body];
    const f3 pos = from4(a.org[body]);
    dr::RayHit h;
    if (st == dc::SHAPE_PLANE) h = dr::ray_plane(sh, p0, p1);
    else if (st == dc::SHAPE_SPHERE) h = dr::ray_sphere(sh.x, pos, p0, p1);
    else {
        const q4 orn = q_from4(a.xf[8 * (size_t)body + 1]);
        if (st == dc::SHAPE_BOX) h = dr::ray_box(from4(sh), pos, orn, p0, p1);
        else if (st == dc::SHAPE_CAPSULE) h = dr::ray_capsule(sh, pos, orn, p0, p1);
        else if (st == dc::SHAPE_CYLINDER) h = dr::ray_cylinder(sh, pos, orn, p0, p1);
        else h = dr::ray_polyhedron(a.meshes, sh, pos, orn, p0, p1);
    }
    if (h.fraction < best.h.fraction || (h.fraction == best.h.fraction && best.body != kNoBody && body < best.body)) { best.h = h; best.body = body; }
}

// One ray: the planes, then the tree along the ropes (or every body), and the record of the best hit.
template <bool kList>
DI void rc_trace(const RayArgs &a, uint32_t r, const float4 *__restrict__ P0, const float4 *__restrict__ P1, uint4 *__restrict__ out,
                 const uint32_t *lst, uint32_t len) {
    const f3 p0 = from4(P0[r]), p1 = from4(P1[r]);
    Best best{dr::ray_miss(), kNoBody};
    if (a.brute) {
        for (uint32_t b = 0; b < a.n_bodies; ++b) rc_candidate<kList>(a, b, p0, p1, best, lst, len);
    } else {
        for (uint32_t k = 0; k < a.n_planes; ++k) rc_candidate<kList>(a, a.planes[k], p0, p1, best, lst, len);
        const float tol = kNodeGrow * (1.0f + max_abs(p0, p1));
        uint32_t node = a.n_tree ? 0u : kRayEnd;   // the root: internal node 0, or leaf 0 of a one-body tree
        while (node != kRayEnd) {
            const float4 lo = a.nmin[node], hi = a.nmax[node];
            const uint32_t w = __float_as_uint(lo.w);
            if (w & kLeafBit) {
                rc_candidate<kList>(a, w & ~kLeafBit, p0, p1, best, lst, len);   // the exact predicate on the body's own box
                node = __float_as_uint(hi.w);
            } else if (dr::intersect_segment_aabb(p0, p1, mk3(lo.x - tol, lo.y - tol, lo.z - tol), mk3(hi.x + tol, hi.y + tol, hi.z + tol))) {
                node = w;
            } else {
                node = __float_as_uint(hi.w);
            }
        }
    }
    const dr::RayHit &h = best.h;
    out[2 * (size_t)r] = make_uint4(best.body, __float_as_uint(h.fraction), __float_as_uint(h.normal.x), __float_as_uint(h.normal.y));
    out[2 * (size_t)r + 1] = make_uint4(__float_as_uint(h.normal.z), (uint32_t)h.feature, h.index, 0u);
}

__global__ void __launch_bounds__(256) k_rc_trace(RayArgs a, uint32_t n, const float4 *__restrict__ P0, const float4 *__restrict__ P1, uint4 *__restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    rc_trace<false>(a, r, P0, P1, out, nullptr, 0u);
}
// The tickets' rays: ray r ignores ign_ids[ign_off[r] .. ign_off[r + 1]) (a.ignore is not read). `out` may be pinned host memory.
__global__ void __launch_bounds__(256) k_rc_trace_lists(RayArgs a, uint32_t n, const float4 *__restrict__ P0, const float4 *__restrict__ P1, uint4 *__restrict__ out,
                                                        const uint32_t *__restrict__ ign_off, const uint32_t *__restrict__ ign_ids) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t lo = ign_off[r], hi = ign_off[r + 1];
    rc_trace<true>(a, r, P0, P1, out, ign_ids + lo, hi - lo);
}

__global__ void k_rc_fill_u32(uint32_t *p, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

static inline uint32_t nblocks(uint32_t n, uint32_t bs) { return (n + bs - 1) / bs; }

// Buffers on first use; boxes and tree when the state moved on since they were built; the ignore bits of this call.
static int prepare(edynhip_ctx *c, uint32_t num_ignore, const uint32_t *ignore, bool &use_mask) {
    if (!c->ray) c->ray = new RayTree();
    RayTree &t = *c->ray;
    const uint32_t cap = c->b.cap;
    if (t.cap != cap) {
        for (void *p : t.allocs) (void)hipFree(p);
        t = RayTree();
        t.cap = cap;
        const size_t nn = 2 * (size_t)cap;
        EH_TRY(ralloc(c, t, t.org, cap)); EH_TRY(ralloc(c, t, t.amin, cap)); EH_TRY(ralloc(c, t, t.amax, cap));
        EH_TRY(ralloc(c, t, t.list, cap)); EH_TRY(ralloc(c, t, t.keys, cap)); EH_TRY(ralloc(c, t, t.keys_sorted, cap));
        EH_TRY(ralloc(c, t, t.parent, nn)); EH_TRY(ralloc(c, t, t.left, nn)); EH_TRY(ralloc(c, t, t.right, nn));
        EH_TRY(ralloc(c, t, t.visit, nn)); EH_TRY(ralloc(c, t, t.rope, nn));
        EH_TRY(ralloc(c, t, t.nmin, nn)); EH_TRY(ralloc(c, t, t.nmax, nn));
        EH_TRY(ralloc(c, t, t.cnt, 1)); EH_TRY(ralloc(c, t, t.mask, cap / 32 + 1));
    }
    const uint32_t n = c->b.n;
    if (t.epoch != c->state_epoch) {
        t.host_list.clear();
        // (a shard of a multi-device world: the bodies another shard answers for stay out of the tree and of the plane list)
        auto mine = [&](uint32_t i) { return c->host_answers.empty() || ((c->host_answers[i >> 5] >> (i & 31u)) & 1u); };
        for (uint32_t i = 0; i < n; ++i)
            if (c->host_shape[i] != EDYNHIP_SHAPE_NONE && c->host_shape[i] != EDYNHIP_SHAPE_PLANE && mine(i)) t.host_list.push_back(i);
        t.n_tree = (uint32_t)t.host_list.size();
        for (uint32_t i = 0; i < n; ++i)
            if (c->host_shape[i] == EDYNHIP_SHAPE_PLANE && mine(i)) t.host_list.push_back(i);
        t.n_planes = (uint32_t)t.host_list.size() - t.n_tree;
        if (n) hipLaunchKernelGGL(k_rc_boxes, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->b, c->meshes, t.org, t.amin, t.amax);
        if (!t.host_list.empty())   // (pageable source: the copy has read it when the call returns)
            EH_HIP(c, hipMemcpyAsync(t.list, t.host_list.data(), t.host_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (t.n_tree) {
            const uint32_t nt = t.n_tree;
            hipLaunchKernelGGL(k_rc_fill_u32, dim3(nblocks(2 * nt - 1, 256)), dim3(256), 0, c->stream, t.parent, 2 * nt - 1, 0xFFFFFFFFu);
            EH_TRY(build_query_tree(c, t.list, nt, t.amin, t.amax, t.cnt, t.keys, t.keys_sorted, t.parent, t.left, t.right, t.visit, t.rope));
            hipLaunchKernelGGL(k_rc_refit, dim3(nblocks(nt, 256)), dim3(256), 0, c->stream, nt, t.keys_sorted, t.parent, t.left, t.right, t.rope,
                               t.amin, t.amax, t.nmin, t.nmax, t.visit);
        }
        EH_HIP(c, hipGetLastError());
        t.epoch = c->state_epoch;
    }
    use_mask = num_ignore > 0;
    if (use_mask) {
        t.host_mask.assign(n / 32 + 1, 0u);
        for (uint32_t k = 0; k < num_ignore; ++k)
            if (ignore[k] < n) t.host_mask[ignore[k] >> 5] |= 1u << (ignore[k] & 31u);
        EH_HIP(c, hipMemcpyAsync(t.mask, t.host_mask.data(), t.host_mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    return EDYNHIP_OK;
}

// query_aabb.hip walks the same tree: boxes and tree brought up to date, no ignore bits.
int query_tree_prepare(edynhip_ctx *c) {
    bool use_mask = false;
    return prepare(c, 0, nullptr, use_mask);
}

static RayArgs ray_args(edynhip_ctx *c, bool use_mask, uint32_t flags) {
    const RayTree &t = *c->ray;
    RayArgs a;
    a.xf = c->b.xf; a.flags = c->b.flags; a.shape = c->b.shape; a.org = t.org; a.amin = t.amin; a.amax = t.amax;
    a.meshes = c->meshes; a.nmin = t.nmin; a.nmax = t.nmax; a.n_tree = t.n_tree;
    a.planes = t.list + t.n_tree; a.n_planes = t.n_planes; a.n_bodies = c->b.n;
    a.ignore = use_mask ? t.mask : nullptr;
    a.answers = c->answers;
    a.brute = (flags & EDYNHIP_RAYCAST_BRUTE_FORCE) ? 1u : 0u;
    return a;
}

static int launch(edynhip_ctx *c, const RayArgs &a, uint32_t n, const float4 *p0, const float4 *p1, uint4 *out) {
    if (n) hipLaunchKernelGGL(k_rc_trace, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, a, n, p0, p1, out);
    EH_HIP(c, hipGetLastError());
    return EDYNHIP_OK;
}

static int raycast_device(edynhip_ctx *c, uint32_t n, const void *p0_f4, const void *p1_f4, uint32_t num_ignore, const uint32_t *ignore,
                          uint32_t flags, void *out) {
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    bool use_mask = false;
    EH_TRY(prepare(c, num_ignore, ignore, use_mask));
    const RayArgs a = ray_args(c, use_mask, flags);
    const float4 *P0 = (const float4 *)p0_f4, *P1 = (const float4 *)p1_f4;
    uint4 *O = (uint4 *)out;
    for (uint32_t off = 0; off < n; off += kChunk)
        EH_TRY(launch(c, a, std::min(kChunk, n - off), P0 + off, P1 + off, O + 2 * (size_t)off));
    return EDYNHIP_OK;
}

// A ticket's rays (query_async.hip): device arrays, ray r with the ignore list ign_ids[ign_off[r] .. ign_off[r + 1]) of its own
// (ign_off == nullptr: no lists); enqueued on the context's stream. The call's bit mask (RayTree::mask) is neither written nor read.
int ticket_trace(edynhip_ctx *c, uint32_t n, const float4 *p0, const float4 *p1, const uint32_t *ign_off, const uint32_t *ign_ids, uint32_t flags, uint4 *out) {
    if (n == 0) return EDYNHIP_OK;
    bool use_mask = false;
    EH_TRY(prepare(c, 0, nullptr, use_mask));
    const RayArgs a = ray_args(c, false, flags);
    for (uint32_t off = 0; off < n; off += kChunk) {
        const uint32_t m = std::min(kChunk, n - off);
        if (!ign_off) { EH_TRY(launch(c, a, m, p0 + off, p1 + off, out + 2 * (size_t)off)); continue; }
        hipLaunchKernelGGL(k_rc_trace_lists, dim3(nblocks(m, 256)), dim3(256), 0, c->stream, a, m, p0 + off, p1 + off, out + 2 * (size_t)off, ign_off + off, ign_ids);
        EH_HIP(c, hipGetLastError());
    }
    return EDYNHIP_OK;
}

void shard_set_answers(edynhip_ctx *c, const uint32_t *answers_dev, std::vector<uint32_t> host_bits, const uint32_t *query_island_dev) {
    c->answers = answers_dev;
    c->host_answers = std::move(host_bits);
    c->query_island = query_island_dev;
    ++c->state_epoch;   // the query tree and the island boxes hold what the context answered for before
}

int shard_raycast(edynhip_ctx *c, uint32_t n, const void *p0_f4, const void *p1_f4, uint32_t num_ignore, const uint32_t *ignore, uint32_t flags, void *out) {
    return raycast_device(c, n, p0_f4, p1_f4, num_ignore, ignore, flags, out);
}

}  // namespace eh

using namespace eh;
// Unknown flag bits and shard contexts (edynhip_world_context) are rejected: a world asks its shards through eh::shard_raycast
// (edynhip_world_raycast, multi_query.hip).
static int check_call(edynhip_ctx *c, uint32_t flags, const char *who) {
    if (flags & ~(uint32_t)EDYNHIP_RAYCAST_BRUTE_FORCE) return set_error(c, EDYNHIP_ERR_INVALID, (std::string(who) + ": unknown flag bits").c_str());
    if (c->world_shard) return set_error(c, EDYNHIP_ERR_UNSUPPORTED, (std::string(who) + ": a shard of a multi-device world has no raycast").c_str());
    return EDYNHIP_OK;
}
static_assert(sizeof(edynhip_raycast_hit) == 32, "edynhip_raycast_hit is 32 bytes");

int edynhip_raycast(edynhip_ctx *c, uint32_t n, const float *p0, const float *p1, uint32_t num_ignore, const uint32_t *ignore,
                    uint32_t flags, edynhip_raycast_hit *out) {
    if (!c || (n && (!p0 || !p1 || !out)) || (num_ignore && !ignore)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_call(c, flags, "edynhip_raycast"));
    if (n == 0) return EDYNHIP_OK;
    EH_HIP(c, hipSetDevice(c->device));
    bool use_mask = false;
    EH_TRY(prepare(c, num_ignore, ignore, use_mask));
    RayTree &t = *c->ray;
    if (!t.stage) EH_TRY(ralloc(c, t, t.stage, 4 * (size_t)kChunk));
    const RayArgs a = ray_args(c, use_mask, flags);
    t.host_pts.resize(2 * (size_t)kChunk);
    for (uint32_t off = 0; off < n; off += kChunk) {
        const uint32_t m = std::min(kChunk, n - off);
        for (uint32_t r = 0; r < m; ++r) {
            const float *q0 = p0 + 3 * ((size_t)off + r), *q1 = p1 + 3 * ((size_t)off + r);
            t.host_pts[r] = make_float4(q0[0], q0[1], q0[2], 0.0f);
            t.host_pts[kChunk + r] = make_float4(q1[0], q1[1], q1[2], 0.0f);
        }
        EH_HIP(c, hipMemcpyAsync(t.stage, t.host_pts.data(), (size_t)m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        EH_HIP(c, hipMemcpyAsync(t.stage + kChunk, t.host_pts.data() + kChunk, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        EH_TRY(launch(c, a, m, t.stage, t.stage + kChunk, (uint4 *)(t.stage + 2 * (size_t)kChunk)));
        EH_HIP(c, hipMemcpyAsync(out + off, t.stage + 2 * (size_t)kChunk, (size_t)m * sizeof(edynhip_raycast_hit), hipMemcpyDeviceToHost, c->stream));
        EH_HIP(c, hipStreamSynchronize(c->stream));   // the staging buffers are reused by the next chunk
    }
    return EDYNHIP_OK;
}

int edynhip_raycast_device(edynhip_ctx *c, uint32_t n, const void *p0_f4, const void *p1_f4, uint32_t num_ignore, const uint32_t *ignore,
                           uint32_t flags, void *out) {
    if (!c || (n && (!p0_f4 || !p1_f4 || !out)) || (num_ignore && !ignore)) return EDYNHIP_ERR_INVALID;
    EH_TRY(check_call(c, flags, "edynhip_raycast_device"));
    return raycast_device(c, n, p0_f4, p1_f4, num_ignore, ignore, flags, out);
}
