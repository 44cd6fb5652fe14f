// The host rules of the single-context C-ABI (capi.hip, capi_scene.hip, capi_readback.hip), each written once: how the joints are
// coloured and packed, how many rows a joint has, the hinge's tangent frame, a body's exclusion list, the default should_collide,
// the canonical key that orders manifold records, and who takes part in the broadphase. Plain C++ over arrays - no HIP, no context -
// so every rule is tested on a machine without a GPU (tests/cpp/ctx_rules.cpp).
#pragma once
#include "../../include/edynhip.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#ifdef __HIPCC__
#define EH_RULE_HD __host__ __device__
#else
#define EH_RULE_HD
#endif

namespace eh {

// ------------------------------------------------------------------------------------------------ joints
constexpr uint32_t kJointNoColour = 0xFFu, kJointMaxColours = 64;   // (ctx.hpp kNoColour, kMaxColours)

// Deterministic edge colouring of the live joints, the rule of the per-step contact colouring (colouring.hip k_col_*): in every round
// each dynamic body nominates the uncoloured joint of the lowest caller index among its own; a joint nominated by all of its dynamic
// ends takes the lowest colour free at those ends. A body that is not dynamic constrains nothing: any number of joints may share a
// colour on it. body[2 e], body[2 e + 1]: the ends of joint e, in caller order; dynamic[b] != 0: body b is dynamic.
// false: a joint found all 64 colours taken ("more than 64 joint colours").
inline bool colour_joints(uint32_t n, const uint32_t *body, const std::vector<uint8_t> &dynamic, std::vector<uint32_t> &colour) {
    colour.assign(n, kJointNoColour);
    std::vector<uint64_t> used(dynamic.size(), 0), best(dynamic.size(), 0);
    for (;;) {
        bool any = false;
        for (uint32_t e = 0; e < n; ++e) {
            if (colour[e] != kJointNoColour) continue;
            any = true;
            const uint64_t pr = (uint64_t)(0xFFFFFFFFu - e);
            const uint32_t a = body[2 * e], b = body[2 * e + 1];
            if (dynamic[a]) best[a] = std::max(best[a], pr);
            if (dynamic[b]) best[b] = std::max(best[b], pr);
        }
        if (!any) break;
        for (uint32_t e = 0; e < n; ++e) {
            if (colour[e] != kJointNoColour) continue;
            const uint64_t pr = (uint64_t)(0xFFFFFFFFu - e);
            const uint32_t a = body[2 * e], b = body[2 * e + 1];
            const bool da = dynamic[a], db = dynamic[b];
            if ((da && best[a] != pr) || (db && best[b] != pr)) continue;
            const uint64_t busy = (da ? used[a] : 0) | (db ? used[b] : 0);
            uint32_t col = 0;
            while (col < kJointMaxColours && (busy >> col & 1)) ++col;
            if (col >= kJointMaxColours) return false;
            colour[e] = col;
            if (da) used[a] |= 1ull << col;
            if (db) used[b] |= 1ull << col;
        }
        std::fill(best.begin(), best.end(), 0);
    }
    return true;
}
// The joints by ascending colour, caller order kept inside a colour: order[p] = the joint at packed position p;
// colour_start[k] = the first position whose colour is at least k, for k = 0 .. number of colours (the trailing entry is n).
// Returns the number of colours; entries of colour_start beyond it are left alone.
inline uint32_t colour_sorted_order(const std::vector<uint32_t> &colour, std::vector<uint32_t> &order, uint32_t *colour_start) {
    const uint32_t n = (uint32_t)colour.size();
    order.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return colour[x] < colour[y]; });
    uint32_t ncol = 0;
    for (uint32_t p = 0; p < n; ++p) ncol = std::max(ncol, colour[order[p]] + 1);
    for (uint32_t k = 0; k <= ncol; ++k) {
        uint32_t q = 0;
        while (q < n && colour[order[q]] < k) ++q;
        colour_start[k] = q;
    }
    return ncol;
}
// Constraint rows a joint of this type prepares at most (its impulse slots in use): point and every other type 3.
inline uint32_t joint_row_count(int32_t type) {
    return type == EDYNHIP_JOINT_HINGE ? 5 : type == EDYNHIP_JOINT_CONE ? 2 : type == EDYNHIP_JOINT_CVJOINT ? 9 : type == EDYNHIP_JOINT_GENERIC ? 24 : 3;
}
// Two unit vectors p, q, orthogonal to each other, that span the plane orthogonal to the unit vector n (geom.cpp:730-754, fp32 on
// the host): built from n's y and z where |n.z| exceeds sqrt(1/2), from its x and y otherwise
constexpr float kRuleHalfSqrt2 = 0.7071067811865475244008443621048490f;   // (dmath.hpp kHalfSqrt2)
inline void plane_space_h(const float *nn, float *p, float *q) {
    if (std::fabs(nn[2]) > kRuleHalfSqrt2) {
        float a = nn[1] * nn[1] + nn[2] * nn[2]; float k = 1.0f / std::sqrt(a);
        p[0] = 0; p[1] = -nn[2] * k; p[2] = nn[1] * k; q[0] = a * k; q[1] = -nn[0] * p[2]; q[2] = nn[0] * p[1];
    } else {
        float a = nn[0] * nn[0] + nn[1] * nn[1]; float k = 1.0f / std::sqrt(a);
        p[0] = -nn[1] * k; p[1] = nn[0] * k; p[2] = 0; q[0] = -nn[2] * p[1]; q[1] = nn[2] * p[0]; q[2] = a * k;
    }
}

// ------------------------------------------------------------------------------------------------ exclusion lists
// A body's collision exclusions (util/exclude_collision.cpp:9-71): 16 entries (collision_exclusion::max_exclusions), the live ones
// first, the rest ~0u. The lists are one way: excluding a pair edits the lists of both bodies.
constexpr uint32_t kExclCap = 16, kExclNone = 0xFFFFFFFFu;
inline bool excl_add(uint32_t *l, uint32_t y) {   // exclude_collision_one_way; false: the list is full (and unchanged)
    uint32_t k = 0;
    for (; k < kExclCap && l[k] != kExclNone; ++k) if (l[k] == y) return true;
    if (k == kExclCap) return false;
    l[k] = y;
    return true;
}
inline void excl_drop(uint32_t *l, uint32_t y) {   // remove_collision_exclusion_one_way: the last entry takes the hole
    uint32_t size = 0;
    while (size < kExclCap && l[size] != kExclNone) ++size;
    for (uint32_t i = size; i; --i)
        if (l[i - 1] == y) { l[i - 1] = l[size - 1]; l[size - 1] = kExclNone; break; }
}
inline bool excl_listed(const uint32_t *l, uint32_t y) {
    for (uint32_t k = 0; k < kExclCap && l[k] != kExclNone; ++k) if (l[k] == y) return true;
    return false;
}
// should_collide_default (should_collide.cpp:11-57): not a body with itself, each body's group in the other's mask, neither body on
// the other's exclusion list. group / mask: per body (a body beyond them has every bit set); excl: [bodies][16], or empty: no lists.
inline int should_collide_default(uint32_t a, uint32_t b, const std::vector<uint64_t> &group, const std::vector<uint64_t> &mask, const std::vector<uint32_t> &excl) {
    if (a == b) return 0;
    if (a < group.size() && b < group.size() && ((group[a] & mask[b]) == 0 || (group[b] & mask[a]) == 0)) return 0;
    if (!excl.empty() && (excl_listed(&excl[(size_t)a * kExclCap], b) || excl_listed(&excl[(size_t)b * kExclCap], a))) return 0;
    return 1;
}

// ------------------------------------------------------------------------------------------------ pairs
// Owner of a pair (see broadphase.hip): the procedural body, the higher index if both are.
EH_RULE_HD inline uint32_t pair_owner(uint32_t a, uint32_t b, bool proc_a, bool proc_b) {
    if (proc_a && proc_b) return a > b ? a : b;
    return proc_a ? a : b;
}
// The canonical key of a pair, owner << 32 | other: manifold records travel in ascending order of it
inline uint64_t canonical_pair_key(uint32_t a, uint32_t b, bool proc_a, bool proc_b) {
    const uint32_t o = pair_owner(a, b, proc_a, proc_b);
    return ((uint64_t)o << 32) | (o == a ? b : a);
}
template <typename KeyAt>
inline bool strictly_ascending(uint32_t n, KeyAt key) {   // key(i) for i < n; equal neighbours are not ascending
    for (uint32_t i = 1; i < n; ++i) if (!(key(i - 1) < key(i))) return false;
    return true;
}
// Broadphase participants from the bodies' (kind, shape): the shaped bodies, [non-procedural ..., procedural ...], each part in
// index order; a body is procedural when it is dynamic. num_np: the length of the first part.
inline std::vector<uint32_t> broadphase_participants(const std::vector<int32_t> &kind, const std::vector<int32_t> &shape, uint32_t &num_np) {
    std::vector<uint32_t> np_list, proc_list;
    for (uint32_t i = 0; i < (uint32_t)kind.size(); ++i) {
        if (shape[i] == EDYNHIP_SHAPE_NONE) continue;
        (kind[i] == EDYNHIP_KIND_DYNAMIC ? proc_list : np_list).push_back(i);
    }
    num_np = (uint32_t)np_list.size();
    np_list.insert(np_list.end(), proc_list.begin(), proc_list.end());
    return np_list;
}

// ------------------------------------------------------------------------------------------------ body edits
// What edynhip_edit_bodies refuses, decided before anything on the device changes. removed[b] != 0: index b is a tombstone
// (edynhip_remove_bodies); num_meshes: the convex meshes the context holds. Returns EDYNHIP_OK or the status of the first fault found,
// with *why (a literal) saying which. The faults, in the order they are looked for: a mask beyond the five groups or a missing array
// (INVALID); an index out of range, a tombstone, an index listed twice (INVALID); INERTIA to be derived (has_inertia 0) without MASS
// (INVALID); a shape type outside box .. polyhedron (UNSUPPORTED); a polyhedron whose shape_param[0] is no mesh id (INVALID); a kind
// that is none (INVALID); a body made dynamic without MASS and INERTIA in the same call (INVALID).
constexpr uint32_t kEditGroups = EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA | EDYNHIP_EDIT_MATERIAL | EDYNHIP_EDIT_SHAPE | EDYNHIP_EDIT_KIND;
inline int validate_body_edit(uint32_t n, const uint32_t *indices, const edynhip_bodies *v, uint32_t fields, uint32_t num_bodies,
                              const std::vector<uint8_t> &removed, uint32_t num_meshes, const char **why) {
    auto fail = [&](int code, const char *msg) { if (why) *why = msg; return code; };
    if (fields & ~kEditGroups) return fail(EDYNHIP_ERR_INVALID, "unknown field group");
    if (n == 0) return EDYNHIP_OK;
    if (!indices || !v) return fail(EDYNHIP_ERR_INVALID, "missing indices or values");
    if (((fields & EDYNHIP_EDIT_MASS) && !v->mass) || ((fields & EDYNHIP_EDIT_MATERIAL) && (!v->friction || !v->restitution)) ||
        ((fields & EDYNHIP_EDIT_SHAPE) && (!v->shape_type || !v->shape_param)) || ((fields & EDYNHIP_EDIT_KIND) && !v->kind))
        return fail(EDYNHIP_ERR_INVALID, "missing array of a named group");
    for (uint32_t k = 0; k < n; ++k) {
        if (indices[k] >= num_bodies) return fail(EDYNHIP_ERR_INVALID, "index out of range");
        if (indices[k] < removed.size() && removed[indices[k]]) return fail(EDYNHIP_ERR_INVALID, "index of a removed body");
    }
    {   // (sorted copy: the cost follows the edit list, not the world)
        std::vector<uint32_t> sorted(indices, indices + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(EDYNHIP_ERR_INVALID, "index listed twice");
    }
    if (fields & EDYNHIP_EDIT_INERTIA)
        for (uint32_t k = 0; k < n; ++k) {
            const bool given = v->has_inertia && v->has_inertia[k];
            if (given && !v->inertia) return fail(EDYNHIP_ERR_INVALID, "has_inertia set without an inertia array");
            if (!given && !(fields & EDYNHIP_EDIT_MASS)) return fail(EDYNHIP_ERR_INVALID, "an inertia derived from the shape needs MASS in the same call");
        }
    if (fields & EDYNHIP_EDIT_SHAPE)
        for (uint32_t k = 0; k < n; ++k) {
            if (v->shape_type[k] < EDYNHIP_SHAPE_BOX || v->shape_type[k] > EDYNHIP_SHAPE_POLYHEDRON) return fail(EDYNHIP_ERR_UNSUPPORTED, "shape type outside box .. polyhedron");
            const float id = v->shape_param[4 * (size_t)k];
            if (v->shape_type[k] == EDYNHIP_SHAPE_POLYHEDRON && (!(id >= 0) || id != std::floor(id) || id >= (float)num_meshes))
                return fail(EDYNHIP_ERR_INVALID, "polyhedron: shape_param[0] is not the id of a mesh");
        }
    if (fields & EDYNHIP_EDIT_KIND)
        for (uint32_t k = 0; k < n; ++k) {
            if (v->kind[k] < EDYNHIP_KIND_DYNAMIC || v->kind[k] > EDYNHIP_KIND_STATIC) return fail(EDYNHIP_ERR_INVALID, "kind is none of dynamic, kinematic, static");
            if (v->kind[k] == EDYNHIP_KIND_DYNAMIC && (fields & (EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA)) != (EDYNHIP_EDIT_MASS | EDYNHIP_EDIT_INERTIA))
                return fail(EDYNHIP_ERR_INVALID, "a body made dynamic needs MASS and INERTIA in the same call");
        }
    return EDYNHIP_OK;
}

}  // namespace eh
