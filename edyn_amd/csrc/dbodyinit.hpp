// What a body's description derives on the device (rigidbody.cpp:47-131): the local inverse inertia from mass and shape, the world
// inverse inertia from the orientation, the AABB from the pose. Written once: the scene upload (capi_scene.hip k_init_bodies) and the
// edits of a running world (body_edit.hip k_edit_bodies) call the same functions, so both round alike (-ffp-contract=off).
#pragma once
#include "ctx.hpp"
#include "dstep.hpp"
#include "dpolyhedron.hpp"

namespace eh {
using namespace dm;

// moment_of_inertia(shape, mass) as a full tensor (moment_of_inertia.cpp); a shapeless or plane body: scalar_max on the diagonal
__device__ inline m3 shape_inertia(int st, float4 sp, float mass, const dc::Meshes &meshes) {
    m3 I;
    if (st == dc::SHAPE_BOX) {   // moment_of_inertia.cpp:11-17,179-181
        f3 ext = from4(sp) * 2.0f;
        f3 d = 1.0f / 12.0f * mass * mk3(ext.y * ext.y + ext.z * ext.z, ext.z * ext.z + ext.x * ext.x, ext.x * ext.x + ext.y * ext.y);
        I = {{d.x, 0, 0}, {0, d.y, 0}, {0, 0, d.z}};
    } else if (st == dc::SHAPE_SPHERE) {   // :19-21,163-165
        float s = 0.4f * mass * sp.x * sp.x;
        I = {{1 * s, 0 * s, 0 * s}, {0 * s, 1 * s, 0 * s}, {0 * s, 0 * s, 1 * s}};
    } else if (st == dc::SHAPE_CAPSULE) {   // moment_of_inertia.cpp:65-90,171-173, shape_volume.cpp:10-16
        const float kPiF = 3.1415926535897932384626433832795029f;
        const float len = sp.y * 2, radius = sp.x;
        const float cyl_vol = kPiF * radius * radius * len;
        const float sph_vol = kPiF * radius * radius * radius * 4.0f / 3.0f;
        const float total_vol = cyl_vol + sph_vol;
        const float cyl_mass = mass * cyl_vol / total_vol, sph_mass = mass * sph_vol / total_vol;
        const float cyl_xx = 0.5f * cyl_mass * radius * radius;
        const float cyl_yy = 1.0f / 12.0f * cyl_mass * (3.0f * radius * radius + len * len);
        const float sph_inertia = 0.4f * sph_mass * radius * radius;
        // the capsule formula reads the cylinder's vector as (.x axial, .y transverse) although it arrives permuted for
        // the axis (:77-81): reproduced - it is the inertia the reference simulates with
        const f3 cyl = sp.z == 0.0f ? mk3(cyl_xx, cyl_yy, cyl_yy) : (sp.z == 1.0f ? mk3(cyl_yy, cyl_xx, cyl_yy) : mk3(cyl_yy, cyl_yy, cyl_xx));
        const float xx = sph_inertia + cyl.x;
        const float yy_zz = sph_inertia + sph_mass * square(4.0f * len + 3.0f * radius) / 64.0f + cyl.y;
        const f3 d = sp.z == 0.0f ? mk3(xx, yy_zz, yy_zz) : (sp.z == 1.0f ? mk3(yy_zz, xx, yy_zz) : mk3(yy_zz, yy_zz, xx));
        I = {{d.x, 0, 0}, {0, d.y, 0}, {0, 0, d.z}};
    } else if (st == dc::SHAPE_CYLINDER) {   // moment_of_inertia.cpp:27-44,167-169
        const f3 d = dc::cylinder_inertia_diag(dc::cyl_of(sp), mass);
        I = {{d.x, 0, 0}, {0, d.y, 0}, {0, 0, d.z}};
    } else if (st == dc::SHAPE_POLYHEDRON) {   // moment_of_inertia.cpp:93-157,183-185
        I = dc::polyhedron_inertia(meshes, sp, mass);
    } else {
        I = {{kScalarMax, 0, 0}, {0, kScalarMax, 0}, {0, 0, kScalarMax}};
    }
    return I;
}
// shift_moment_of_inertia (moment_of_inertia.cpp:217-220): I + (d^T d) m, d = skew(com)
__device__ inline m3 shift_inertia(m3 I, f3 com, float mass) {
    const m3 d = {{0, -com.z, com.y}, {com.z, 0, -com.x}, {-com.y, com.x, 0}};
    const m3 dd = mul(transpose(d), d);
    return {I.r0 + dd.r0 * mass, I.r1 + dd.r1 * mass, I.r2 + dd.r2 * mass};
}
// inverse_matrix_symmetric, matrix3x3.hpp:190-218
__device__ inline m3 inverse_symmetric(m3 I) {
    m3 il;
    float det = dot(I.r0, cross(I.r1, I.r2));
    float di = 1.0f / det;
    float a11 = I.r0.x, a12 = I.r0.y, a13 = I.r0.z, a22 = I.r1.y, a23 = I.r1.z, a33 = I.r2.z;
    il.r0.x = di * (a22 * a33 - a23 * a23);
    il.r0.y = di * (a13 * a23 - a12 * a33);
    il.r0.z = di * (a12 * a23 - a13 * a22);
    il.r1.x = il.r0.y;
    il.r1.y = di * (a11 * a33 - a13 * a13);
    il.r1.z = di * (a12 * a13 - a11 * a23);
    il.r2.x = il.r0.z;
    il.r2.y = il.r1.z;
    il.r2.z = di * (a11 * a22 - a12 * a12);
    return il;
}
// The local inverse inertia of a dynamic body: the caller's tensor (given != nullptr: 9 floats, row-major), or the shape's, shifted to
// the centre of mass where the body has an offset
__device__ inline m3 local_inertia_inv(const float *given, int st, float4 sp, float mass, f3 com, bool has_com, const dc::Meshes &meshes) {
    m3 I;
    if (given) I = {{given[0], given[1], given[2]}, {given[3], given[4], given[5]}, {given[6], given[7], given[8]}};
    else I = shape_inertia(st, sp, mass, meshes);
    if (has_com && !given) I = shift_inertia(I, com, mass);
    return inverse_symmetric(I);
}
__device__ inline m3 world_inertia_inv(m3 il, q4 orn) {
    m3 basis = to_m3(orn);
    return mul(mul(basis, il), transpose(basis));
}
// shape_aabb (aabb_util.cpp:11-70); pos: where the shape is anchored (the body's origin)
__device__ inline void shape_aabb(int st, float4 sp, f3 pos, q4 orn, const dc::Meshes &meshes, f3 &mn, f3 &mx) {
    mn = pos; mx = pos;
    if (st == dc::SHAPE_BOX) {
        const m3 basis = to_m3(orn);
        const f3 h = from4(sp);
        float lo[3] = {pos.x, pos.y, pos.z}, hi[3] = {pos.x, pos.y, pos.z};
        const f3 rws[3] = {basis.r0, basis.r1, basis.r2};
        for (int rr = 0; rr < 3; ++rr)
            for (int cc = 0; cc < 3; ++cc) {
                float e = comp(rws[rr], cc) * -comp(h, cc);
                float f = -e;
                if (e < f) { lo[rr] += e; hi[rr] += f; } else { lo[rr] += f; hi[rr] += e; }
            }
        mn = mk3(lo[0], lo[1], lo[2]); mx = mk3(hi[0], hi[1], hi[2]);
    } else if (st == dc::SHAPE_SPHERE) {
        mn = mk3(pos.x - sp.x, pos.y - sp.x, pos.z - sp.x); mx = mk3(pos.x + sp.x, pos.y + sp.x, pos.z + sp.x);
    } else if (st == dc::SHAPE_CAPSULE) {   // aabb_util.cpp:81-88
        const f3 v = rotate(orn, dc::axis_vector(sp.z)) * sp.y;
        const f3 p0 = pos - v, p1 = pos + v;
        mn = mk3(fminf(p0.x, p1.x) - sp.x, fminf(p0.y, p1.y) - sp.x, fminf(p0.z, p1.z) - sp.x);
        mx = mk3(fmaxf(p0.x, p1.x) + sp.x, fmaxf(p0.y, p1.y) + sp.x, fmaxf(p0.z, p1.z) + sp.x);
    } else if (st == dc::SHAPE_CYLINDER) {   // aabb_util.cpp:72-79
        const box3 bb = dc::cylinder_aabb(dc::cyl_of(sp), pos, orn);
        mn = bb.mn; mx = bb.mx;
    } else if (st == dc::SHAPE_POLYHEDRON) {   // aabb_util.cpp:141-164,195-197
        const box3 bb = dc::polyhedron_aabb(meshes, sp, pos, orn);
        mn = bb.mn; mx = bb.mx;
    } else if (st == dc::SHAPE_PLANE) {
        const f3 nrm = from4(sp);
        f3 umin = mk3(-1, -1, -1), umax = mk3(1, 1, 1);
        if (eq(nrm, mk3(1, 0, 0))) umax = mk3(0, 1, 1);
        else if (eq(nrm, mk3(-1, 0, 0))) umin = mk3(0, -1, -1);
        else if (eq(nrm, mk3(0, 1, 0))) umax = mk3(1, 0, 1);
        else if (eq(nrm, mk3(0, -1, 0))) umin = mk3(-1, 0, -1);
        else if (eq(nrm, mk3(0, 0, 1))) umax = mk3(1, 1, 0);
        else if (eq(nrm, mk3(0, 0, -1))) umin = mk3(-1, -1, 0);
        const f3 pw = nrm * sp.w;
        mn = umin * 99999.0f + pw; mx = umax * 99999.0f + pw;
    }
}

}  // namespace eh
