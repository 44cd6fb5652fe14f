"""Generates tests/golden/raycast_{random,inside,grazing,parallel,plane}.npz: what the reference's own edyn::raycast
(src/edyn/collision/raycast.cpp:20-56, compiled into oracle/_ref/libedynref.so) returns for 20 000 rays of each kind on one scene
built by the real engine (RefWorld) in zero gravity with zero velocities and stepped once, so that no AABB moves and the
reference's fat tree boxes are exactly the AABBs grown by 0.1.

The scene has every shape: a plane, boxes, spheres, capsules and cylinders on all three axes, convex polyhedra (create_mesh with
real=True through RefWorld.add_bodies), centre-of-mass offsets, static and dynamic bodies, nothing touching. Scene and rays are made
from SplitMix64 streams (edyn_amd.scenes.splitmix64_uniform) and float64 arithmetic, so tests rebuild them bit for bit; the files
hold the results only, with a digest of the rays and of the scene they were computed for.

Per ray: entity (0xFFFFFFFF = none; the bodies are entities 0..n-1), fraction, normal, variant index of info_var
(0 monostate, 1 box, 2 cylinder, 3 capsule, 4 polyhedron), feature byte (cylinder / capsule info), index (face / hemisphere;
-1 = SIZE_MAX), and `normal_defined` = 0 where the reference's normal is undefined (a capsule hemisphere reached by a ray parallel
to the axis reads u_in uninitialised, raycast.cpp:214,227-231; a box / polyhedron face index of SIZE_MAX).

Run from the repo root (needs `make -C oracle ref`):  python tests/golden/make_raycast.py
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from edyn_amd import scenes   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("random", "inside", "grazing", "parallel", "plane")
RAYS_PER_KIND = 20000


def _u(count, stream):
    return scenes.splitmix64_uniform(count, stream=stream).astype(np.float64)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rotate(q, v):   # quaternion (x, y, z, w) rotation, float64 (ray construction only)
    r, w = q[:, :3], q[:, 3:4]
    return v + np.cross(2 * r, np.cross(r, v) + w * v)


def scene():
    """Plane at y = 0 plus a 7 x 3 x 7 lattice (pitch 2.5) of the shapes in turn, random orientations."""
    shapes = [(scenes.SHAPE_BOX, (0.5, 0.3, 0.4, 0)), (scenes.SHAPE_SPHERE, (0.45, 0, 0, 0))]
    shapes += [(scenes.SHAPE_CAPSULE, (0.25, 0.4, a, 0)) for a in range(3)] + [(scenes.SHAPE_CYLINDER, (0.3, 0.35, a, 0)) for a in range(3)]
    shapes += [(scenes.SHAPE_POLYHEDRON, (m, 0, 0, 0)) for m in range(6)]
    nx, ny, nz = 7, 3, 7
    n = 1 + nx * ny * nz
    s = scenes._empty(n)
    scenes._add_plane(s)
    s["meshes"] = scenes.convex_library()
    s["com"] = np.zeros((n, 3), np.float32)
    u = _u(4 * n, 101).reshape(n, 4) * 2 - 1
    q = _unit(u).astype(np.float32)
    i = 1
    for y in range(ny):
        for x in range(nx):
            for z in range(nz):
                st, sp = shapes[(i - 1) % len(shapes)]
                s["shape_type"][i] = st
                s["shape_param"][i] = sp
                s["pos"][i] = ((x - 3) * 2.5, 1.5 + 2.5 * y, (z - 3) * 2.5)
                s["orn"][i] = q[i]
                s["kind"][i] = scenes.KIND_STATIC if i % 3 == 0 else scenes.KIND_DYNAMIC
                if i % 11 == 5 and i % 3 != 0:   # (centre-of-mass offsets on dynamic bodies only: apply_center_of_mass needs velocities)
                    s["com"][i] = (0.1, -0.05, 0.03)
                i += 1
    return s


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scene_digest(s):
    return digest(s["kind"], s["pos"], s["orn"], s["shape_type"], s["shape_param"], s["com"])


def rays(kind, s, n=RAYS_PER_KIND):
    """(p0, p1) float32 [n][3] of one kind."""
    k = KINDS.index(kind)
    bodies = np.flatnonzero(s["shape_type"] != scenes.SHAPE_PLANE)
    pos = s["pos"].astype(np.float64)
    u = _u(12 * n, 200 + k).reshape(n, 12)
    pick = bodies[np.minimum((u[:, 0] * len(bodies)).astype(np.int64), len(bodies) - 1)]
    d = _unit(u[:, 1:4] * 2 - 1)
    length = 0.5 + u[:, 4:5] * 19.5
    if kind == "random":
        lo, hi = np.array([-10, -2, -10.0]), np.array([10, 9, 10.0])
        p0 = lo + (hi - lo) * u[:, 5:8]
        p1 = p0 + d * length
    elif kind == "inside":   # from within 0.15 of a body's position, outwards or across
        p0 = pos[pick] + (u[:, 5:8] * 2 - 1) * 0.15
        p1 = p0 + d * (0.1 + u[:, 4:5] * 4.9)
    elif kind == "grazing":
        # half along the box / fat-AABB-like planes of the body frame: a point on a local face plane at half extent 0.5, 0.3, 0.4 or
        # the fat box offset, moving in that plane; half in world axes at the body's position +- its extent
        q = s["orn"][pick].astype(np.float64)
        ax = np.minimum((u[:, 8] * 3).astype(np.int64), 2)
        ext = np.where(u[:, 9:10] < 0.5, np.array([0.5, 0.3, 0.4])[ax][:, None], np.array([0.6, 0.4, 0.5])[ax][:, None])
        local = (u[:, 5:8] * 2 - 1) * 0.8
        sign = np.where(u[:, 10] < 0.5, -1.0, 1.0)
        local[np.arange(n), ax] = sign * ext[:, 0]
        tangent = u[:, 1:4] * 2 - 1
        tangent[np.arange(n), ax] = 0
        tangent = _unit(tangent)
        world = u[:, 11] < 0.5
        p0 = np.where(world[:, None], pos[pick] + local, pos[pick] + _rotate(q, local))
        dd = np.where(world[:, None], tangent, _rotate(q, tangent))
        p0 = p0 - dd * 1.5
        p1 = p0 + dd * 3.0
    elif kind == "parallel":   # along a world axis, or along one of the body's own axes (capsule / cylinder axes, box faces)
        q = s["orn"][pick].astype(np.float64)
        ax = np.minimum((u[:, 8] * 3).astype(np.int64), 2)
        e = np.zeros((n, 3)); e[np.arange(n), ax] = np.where(u[:, 10] < 0.5, -1.0, 1.0)
        dd = np.where((u[:, 11] < 0.5)[:, None], e, _rotate(q, e))
        off = (u[:, 5:8] * 2 - 1) * 0.5
        off = off - dd * np.sum(off * dd, axis=1, keepdims=True)   # sideways offset only
        p0 = pos[pick] + off - dd * 2.0
        p1 = p0 + dd * (1.0 + u[:, 4:5] * 3.0)
    else:   # "plane": crossing y = 0 downwards and upwards, and starting just above / below it
        p0 = np.stack([(u[:, 5] * 2 - 1) * 10, (u[:, 6] * 2 - 1) * 3, (u[:, 7] * 2 - 1) * 10], axis=1)
        p1 = p0 + d * length
        flip = u[:, 9] < 0.5
        p1[:, 1] = np.where(flip, -p0[:, 1] * (0.5 + u[:, 10]), p1[:, 1])
        near = u[:, 11] < 0.25
        p0[:, 1] = np.where(near, (u[:, 8] * 2 - 1) * 1e-3, p0[:, 1])
    return p0.astype(np.float32), p1.astype(np.float32)


class _V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class _Vec(C.Structure):   # std::vector<entt::entity>: begin, end, capacity
    _fields_ = [("b", C.c_void_p), ("e", C.c_void_p), ("c", C.c_void_p)]


class _Hit(C.Structure):   # raycast_result: shape_raycast_result (56 B) + entity
    _fields_ = [("fraction", C.c_float), ("normal", C.c_float * 3), ("storage", C.c_uint8 * 32), ("index", C.c_uint8),
                ("pad", C.c_uint8 * 7), ("entity", C.c_uint32), ("pad2", C.c_uint32)]


def reference_world(s):
    from oracle import binding as ob
    r = ob.RefWorld(gravity=(0, 0, 0))
    r.add_bodies(s)
    r.step(1)
    return r


def reference_raycast(r, p0, p1):
    """edyn::raycast(registry, p0, p1, {}) for every ray: a structured array as the fixtures hold it."""
    f = r.L._ZN4edyn7raycastERN4entt8registryENS_7vector3ES3_RKSt6vectorINS0_6entityESaIS5_EE
    f.restype = _Hit
    f.argtypes = [C.c_void_p, _V3, _V3, C.POINTER(_Vec)]   # the registry is RefWorld's first member (ref_world.cpp)
    empty = _Vec(None, None, None)
    out = np.zeros(len(p0), RESULT_DTYPE)
    for i in range(len(p0)):
        h = f(r.h, _V3(*map(float, p0[i])), _V3(*map(float, p1[i])), C.byref(empty))
        st = bytes(h.storage)
        v = h.index
        feat, idx = 0, 0
        if v in (1, 4):
            idx = int.from_bytes(st[0:8], "little", signed=True)
        elif v in (2, 3):
            feat, idx = st[0], int.from_bytes(st[8:16], "little", signed=True)
        out[i] = (h.entity, h.fraction, tuple(h.normal), v, feat, idx, 1)
    return out


RESULT_DTYPE = np.dtype([("entity", np.uint32), ("fraction", np.float32), ("normal", np.float32, 3), ("variant", np.uint8),
                         ("feature", np.uint8), ("index", np.int32), ("normal_defined", np.uint8)])


def mark_undefined(res, s, p0, p1):
    """normal_defined = 0 where the reference's normal is undefined (see the module docstring)."""
    res = res.copy()
    res["normal_defined"][(res["variant"] == 1) & (res["index"] < 0)] = 0
    res["normal_defined"][(res["variant"] == 4) & (res["index"] < 0)] = 0
    cap = np.flatnonzero((res["variant"] == 3) & (res["feature"] == 0))
    for i in cap:   # closest_point_line_line's parallel test (geom.cpp:46-69), evaluated in float32 on the capsule's axis
        b = int(res["entity"][i])
        q = s["orn"][b:b + 1].astype(np.float32)
        e = np.zeros((1, 3), np.float32); e[0, int(s["shape_param"][b][2])] = 1
        ax = (_rotate(q.astype(np.float64), e.astype(np.float64))[0] * 2 * s["shape_param"][b][1]).astype(np.float32)
        d2 = (p1[i] - p0[i]).astype(np.float32)
        a, bb, ee = np.dot(ax, ax), np.dot(ax, d2), np.dot(d2, d2)
        if not (np.float32(a * ee - bb * bb) > np.float32(np.finfo(np.float32).eps) * 64):
            res["normal_defined"][i] = 0
    return res


def main():
    s = scene()
    r = reference_world(s)
    for kind in KINDS:
        p0, p1 = rays(kind, s)
        res = mark_undefined(reference_raycast(r, p0, p1), s, p0, p1)
        path = os.path.join(HERE, f"raycast_{kind}.npz")
        np.savez_compressed(path, result=res, rays_sha256=digest(p0, p1), scene_sha256=scene_digest(s))
        hit = res["entity"] != 0xFFFFFFFF
        print(kind, "hits", int(hit.sum()), "variants", np.bincount(res["variant"][hit], minlength=5).tolist(),
              "negative", int((res["fraction"][hit] < 0).sum()), "undefined normals", int((res["normal_defined"] == 0).sum()),
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
