// Device raycast routines: the reference's shape_raycast overloads (src/edyn/collision/raycast.cpp) and the geometry they use
// (src/edyn/math/geom.cpp), operation for operation. Built with -ffp-contract=off like every kernel here, so they round like
// the reference's scalar C++. std::max / std::min are written out as the ternaries they are (their NaN behaviour differs
// from fmaxf / fminf).
#pragma once
#include "dmath.hpp"
#include "dmesh.hpp"
#include "../../include/edynhip.h"

namespace dr {
using namespace dm;

struct RayHit {
    float fraction;
    f3 normal;
    int32_t feature;        // EDYNHIP_RAYCAST_FEATURE_*
    uint32_t index;         // face / hemisphere index of the feature (~0u: the reference's SIZE_MAX)
};
DI RayHit ray_miss() { return RayHit{kScalarMax, mk3(0, 0, 0), EDYNHIP_RAYCAST_FEATURE_NONE, 0u}; }
DI f3 axis_vec3(float axis) { return axis == 0.0f ? mk3(1, 0, 0) : (axis == 1.0f ? mk3(0, 1, 0) : mk3(0, 0, 1)); }

// geom.cpp:1185-1223 (Ericson 5.3.3)
DI bool intersect_segment_aabb(f3 p0, f3 p1, f3 mn, f3 mx) {
    const f3 center = (mn + mx) * 0.5f;
    const f3 he = mx - center;
    f3 mid = (p0 + p1) * 0.5f;
    const f3 hl = p1 - mid;
    mid = mid - center;
    f3 ahl = mk3(fabsf(hl.x), fabsf(hl.y), fabsf(hl.z));
    if (fabsf(mid.x) > he.x + ahl.x) return false;
    if (fabsf(mid.y) > he.y + ahl.y) return false;
    if (fabsf(mid.z) > he.z + ahl.z) return false;
    ahl = ahl + mk3(kEps, kEps, kEps);
    if (fabsf(mid.y * hl.z - mid.z * hl.y) > he.y * ahl.z + he.z * ahl.y) return false;
    if (fabsf(mid.z * hl.x - mid.x * hl.z) > he.z * ahl.x + he.x * ahl.z) return false;
    if (fabsf(mid.x * hl.y - mid.y * hl.x) > he.x * ahl.y + he.y * ahl.x) return false;
    return true;
}

// geom.cpp:35-44
DI float closest_point_line(f3 q0, f3 dir, f3 p, float &t, f3 &r) {
    const f3 w = p - q0;
    const float a = dot(w, dir);
    const float b = dot(dir, dir);
    t = a / b;
    r = q0 + dir * t;
    return length_sqr(p - r);
}

// geom.cpp:46-69
DI bool closest_point_line_line(f3 p1, f3 q1, f3 p2, f3 q2, float &s, float &t) {
    const f3 d1 = q1 - p1, d2 = q2 - p2, r = p1 - p2;
    const float a = dot(d1, d1), b = dot(d1, d2), c = dot(d1, r), e = dot(d2, d2), f = dot(d2, r);
    const float d = a * e - b * b;
    if (!(d > kEps)) return false;
    const float d_inv = 1.0f / d;
    s = (b * f - c * e) * d_inv;
    t = (a * f - b * c) * d_inv;
    return true;
}

// geom.cpp:1225-1274; kind: 0 parallel_directions, 1 distance_greater_than_radius, 2 intersects
struct CylRay { int kind; float dist_sqr; f3 normal; };
DI CylRay intersect_ray_cylinder(f3 p0, f3 p1, f3 pos, q4 orn, float radius, float half_length, float axis, float &fraction_in, float &fraction_out) {
    const f3 cyl_dir = rotate(orn, axis_vec3(axis));
    const f3 v0 = pos + cyl_dir * half_length, v1 = pos - cyl_dir * half_length;
    float s, t;
    if (!closest_point_line_line(v0, v1, p0, p1, s, t)) return CylRay{0, 0.0f, mk3(0, 0, 0)};
    const float radius_sqr = square(radius);
    const f3 closest_cyl = lerp(v0, v1, s);
    const f3 closest_ray = lerp(p0, p1, t);
    const f3 normal = closest_ray - closest_cyl;
    const float dist_sqr = length_sqr(normal);
    if (dist_sqr > radius_sqr) return CylRay{1, 0.0f, mk3(0, 0, 0)};
    const f3 d = p1 - p0, e = v1 - v0;
    const float dd = dot(d, d), ee = dot(e, e), de = dot(d, e);
    const float delta_sqr = (radius_sqr - dist_sqr) * ee / (dd * ee - de * de);
    const float delta = sqrtf(delta_sqr);
    fraction_in = t - delta;
    fraction_out = t + delta;
    return CylRay{2, dist_sqr, normal};
}

// geom.cpp:1276-1304 (Ericson 5.3.2)
DI bool intersect_ray_sphere(f3 p0, f3 p1, f3 pos, float radius, float &t) {
    const f3 d = p1 - p0, m = p0 - pos;
    const float a = dot(d, d), b = dot(m, d), c = dot(m, m) - radius * radius;
    if (c > 0 && b > 0) return false;
    const float discr = b * b - a * c;
    if (discr < 0) return false;
    t = (-b - sqrtf(discr)) / a;
    t = 0.0f < t ? t : 0.0f;   // std::max(scalar(0), t)
    return true;
}

// raycast.cpp:58-109. Not clipped to [0, 1]: a ray that starts inside returns a negative fraction. A zero-length ray inside the box
// leaves face_idx = SIZE_MAX (get_face_normal(SIZE_MAX) is undefined there): index ~0u and a zero normal here.
DI RayHit ray_box(f3 h, f3 pos, q4 orn, f3 wp0, f3 wp1) {
    const f3 p0 = to_object(wp0, pos, orn), p1 = to_object(wp1, pos, orn);
    const f3 dir = p1 - p0;
    float t_min = -kScalarMax, t_max = kScalarMax;
    uint32_t face = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (fabsf(dir[i]) < kEps) {
            if (fabsf(p0[i]) > h[i]) return ray_miss();
        } else {
            const float d_inv = 1.0f / dir[i];
            float t1 = (-h[i] - p0[i]) * d_inv;
            float t2 = (+h[i] - p0[i]) * d_inv;
            if (t1 > t2) { const float x = t1; t1 = t2; t2 = x; }
            if (t1 > t_min) face = (uint32_t)(i * 2 + (p0[i] > 0 ? 0 : 1));
            t_min = t_min < t1 ? t1 : t_min;   // std::max(t_min, t1)
            t_max = t2 < t_max ? t2 : t_max;   // std::min(t_max, t2)
            if (t_min > t_max) return ray_miss();
        }
    }
    f3 n = mk3(0, 0, 0);
    if (face != 0xFFFFFFFFu) {   // box_shape.cpp:185-200
        const float s = (face & 1u) ? -1.0f : 1.0f;
        const uint32_t ax = face >> 1;
        n = rotate(orn, mk3(ax == 0 ? s : 0.0f, ax == 1 ? s : 0.0f, ax == 2 ? s : 0.0f));
    }
    return RayHit{t_min, n, EDYNHIP_RAYCAST_FEATURE_BOX_FACE, face};
}

// raycast.cpp:111-180; shape = (radius, half_length, axis)
DI RayHit ray_cylinder(float4 sh, f3 pos, q4 orn, f3 p0, f3 p1) {
    float fraction_in = 0.0f, fraction_out = 0.0f;
    const CylRay res = intersect_ray_cylinder(p0, p1, pos, orn, sh.x, sh.y, sh.z, fraction_in, fraction_out);
    if (res.kind == 1) return ray_miss();
    const f3 dir = rotate(orn, axis_vec3(sh.z));   // cylinder_shape.hpp:33-39
    const f3 v[2] = {pos + dir * sh.y, pos - dir * sh.y};
    const f3 ray_dir = p1 - p0;
    const f3 cyl_dir = v[1] - v[0];
    const f3 cyl_dir_norm = normalize(cyl_dir);
    const uint32_t face_idx = dot(p0 - pos, cyl_dir) < 0 ? 0u : 1u;
    const f3 face_normal = cyl_dir_norm * (face_idx == 0 ? -1.0f : 1.0f);
    const float radius_sqr = square(sh.x);
    if (res.kind == 0) {   // parallel: does the segment cross a cap face?
        f3 closest; float fraction;
        const float dist_sqr = closest_point_line(p0, ray_dir, v[face_idx], fraction, closest);
        if (dist_sqr > radius_sqr) return ray_miss();
        return RayHit{fraction, face_normal, EDYNHIP_RAYCAST_FEATURE_CYLINDER_FACE, face_idx};
    }
    f3 intersection = lerp(p0, p1, fraction_in);
    const float proj0 = dot(intersection - v[0], cyl_dir_norm), proj1 = dot(intersection - v[1], cyl_dir_norm);
    if (proj0 > 0 && proj1 < 0)
        return RayHit{fraction_in, res.normal / sqrtf(res.dist_sqr), EDYNHIP_RAYCAST_FEATURE_CYLINDER_SIDE_EDGE, 0u};
    const float t = dot(v[face_idx] - p0, face_normal) / dot(ray_dir, face_normal);
    intersection = lerp(p0, p1, t);
    if (distance_sqr(intersection, v[face_idx]) > radius_sqr) return ray_miss();
    return RayHit{t, face_normal, EDYNHIP_RAYCAST_FEATURE_CYLINDER_FACE, face_idx};
}

// raycast.cpp:182-195
DI RayHit ray_sphere(float radius, f3 pos, f3 p0, f3 p1) {
    float t;
    if (!intersect_ray_sphere(p0, p1, pos, radius, t)) return ray_miss();
    return RayHit{t, normalize(lerp(p0, p1, t) - pos), EDYNHIP_RAYCAST_FEATURE_NONE, 0u};
}

// raycast.cpp:197-257; shape = (radius, half_length, axis). The hemisphere's normal is taken at lerp(p0, p1, u_in) as in the
// reference; when the ray is parallel to the axis the reference reads u_in uninitialised - here it is the hemisphere's fraction.
DI RayHit ray_capsule(float4 sh, f3 pos, q4 orn, f3 p0, f3 p1) {
    float u_in = 0.0f, u_out = 0.0f;
    const CylRay res = intersect_ray_cylinder(p0, p1, pos, orn, sh.x, sh.y, sh.z, u_in, u_out);
    if (res.kind == 1) return ray_miss();
    const f3 dir = rotate(orn, axis_vec3(sh.z));   // capsule_shape.hpp:21-27
    const f3 v[2] = {pos + dir * sh.y, pos - dir * sh.y};
    const f3 cap_dir = v[1] - v[0];
    const float radius = sh.x;
    uint32_t hemi;
    if (res.kind == 0) {
        hemi = dot(p0 - pos, cap_dir) < 0 ? 0u : 1u;
    } else {
        const f3 intersection = lerp(p0, p1, u_in);
        const float proj0 = dot(intersection - v[0], cap_dir), proj1 = dot(intersection - v[1], cap_dir);
        if (proj0 > 0 && proj1 < 0)
            return RayHit{u_in, res.normal / sqrtf(res.dist_sqr), EDYNHIP_RAYCAST_FEATURE_CAPSULE_SIDE, 0u};
        hemi = proj0 < 0 ? 0u : 1u;
    }
    float fraction;
    if (!intersect_ray_sphere(p0, p1, v[hemi], radius, fraction)) return ray_miss();
    const float u = res.kind == 0 ? fraction : u_in;
    return RayHit{fraction, normalize(lerp(p0, p1, u) - pos), EDYNHIP_RAYCAST_FEATURE_CAPSULE_HEMISPHERE, hemi};
}

// raycast.cpp:259-319 (Ericson 5.3.8) over the body's local convex_mesh (the same tables the narrowphase reads, dpolyhedron.hpp)
DI RayHit ray_polyhedron(const dc::Meshes &t, float4 sh, f3 pos, q4 orn, f3 wp0, f3 wp1) {
    const dc::MeshDesc md = t.desc[(uint32_t)sh.x];
    const f3 p0 = to_object(wp0, pos, orn), p1 = to_object(wp1, pos, orn);
    const f3 d = p1 - p0;
    float t0 = -kScalarMax, t1 = kScalarMax;
    uint32_t face = 0xFFFFFFFFu;
    for (uint32_t f = 0; f < md.nf; ++f) {
        const f3 vertex = from4(t.vertices[md.v_off + t.face_first[md.f_off + f]]);
        const f3 normal = from4(t.normals[md.f_off + f]);
        const float dist = dot(vertex - p0, normal);
        const float denom = dot(normal, d);
        if (fabsf(denom) < kEps) {
            if (dist > 0) return ray_miss();
        } else {
            const float tt = dist / denom;
            if (denom < 0) {
                if (tt > t0) { t0 = tt; face = f; }
            } else {
                if (tt < t1) t1 = tt;
            }
            if (t0 > t1) return ray_miss();
        }
    }
    if ((t0 < 0 && t1 < 0) || (t0 > 1 && t1 > 1)) return ray_miss();
    const f3 n = face != 0xFFFFFFFFu ? rotate(orn, from4(t.normals[md.f_off + face])) : mk3(0, 0, 0);
    return RayHit{clamp_unit(t0), n, EDYNHIP_RAYCAST_FEATURE_POLYHEDRON_FACE, face};
}

// raycast.cpp:356-380; shape = (normal, constant). Not clipped to [0, 1].
DI RayHit ray_plane(float4 sh, f3 p0, f3 p1) {
    const f3 n = from4(sh);
    const f3 c = n * sh.w;
    const float d = dot(p1 - p0, n);
    const float e = dot(c - p0, n);
    if (fabsf(d) < kEps) {
        if (fabsf(e) < kEps) return RayHit{0.0f, n, EDYNHIP_RAYCAST_FEATURE_NONE, 0u};
        return ray_miss();
    }
    return RayHit{e / d, n, EDYNHIP_RAYCAST_FEATURE_NONE, 0u};
}

}  // namespace dr
