"""ctypes access to the reference's own raycast routines in oracle/_ref/libedynref.so (test side only).

edyn::shape_raycast(<shape> const &, raycast_context const &) returns shape_raycast_result (56 B) through a hidden pointer:
fraction at 0, normal at 4, the variant's storage at 16 (the first size_t of box / polyhedron info is the face index; cylinder /
capsule info hold the feature byte at 16 and the index at 24), the variant index byte at 48. raycast_context is pos, orn, p0, p1
(52 B). edyn::intersect_segment_aabb takes four vector3 by value.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libedynref.so")

# variant alternatives of shape_raycast_result::info_var (raycast.hpp:105-114)
V_NONE, V_BOX, V_CYLINDER, V_CAPSULE, V_POLYHEDRON = 0, 1, 2, 3, 4
# EDYNHIP_RAYCAST_FEATURE_* for (variant, feature byte)
FEATURE_OF = {(V_NONE, 0): 0, (V_BOX, 0): 1, (V_CYLINDER, 0): 2, (V_CYLINDER, 1): 3, (V_CAPSULE, 0): 4, (V_CAPSULE, 1): 5,
              (V_POLYHEDRON, 0): 6}


class V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Ctx(C.Structure):   # raycast_context
    _fields_ = [("pos", C.c_float * 3), ("orn", C.c_float * 4), ("p0", C.c_float * 3), ("p1", C.c_float * 3)]


class Result(C.Structure):   # shape_raycast_result
    _fields_ = [("fraction", C.c_float), ("normal", C.c_float * 3), ("storage", C.c_uint8 * 32), ("index", C.c_uint8), ("pad", C.c_uint8 * 7)]


class Box(C.Structure):
    _fields_ = [("half_extents", C.c_float * 3)]


class Sphere(C.Structure):
    _fields_ = [("radius", C.c_float)]


class Axial(C.Structure):   # capsule_shape / cylinder_shape: radius, half_length, axis (unsigned char)
    _fields_ = [("radius", C.c_float), ("half_length", C.c_float), ("axis", C.c_uint8)]


class Plane(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("constant", C.c_float)]


_SYM = {1: ("_ZN4edyn13shape_raycastERKNS_9box_shapeERKNS_15raycast_contextE", Box),
        2: ("_ZN4edyn13shape_raycastERKNS_12sphere_shapeERKNS_15raycast_contextE", Sphere),
        3: ("_ZN4edyn13shape_raycastERKNS_11plane_shapeERKNS_15raycast_contextE", Plane),
        4: ("_ZN4edyn13shape_raycastERKNS_13capsule_shapeERKNS_15raycast_contextE", Axial),
        5: ("_ZN4edyn13shape_raycastERKNS_14cylinder_shapeERKNS_15raycast_contextE", Axial)}


def available():
    return os.path.exists(LIB)


class RefRaycast:
    def __init__(self):
        self.lib = C.CDLL(LIB)
        self.fn = {}
        for st, (name, T) in _SYM.items():
            f = getattr(self.lib, name)
            f.restype = Result
            f.argtypes = [C.POINTER(T), C.POINTER(Ctx)]
            self.fn[st] = (f, T)
        self.seg_aabb = self.lib._ZN4edyn22intersect_segment_aabbENS_7vector3ES0_S0_S0_
        self.seg_aabb.restype = C.c_bool
        self.seg_aabb.argtypes = [V3, V3, V3, V3]

    def intersect_segment_aabb(self, p0, p1, mn, mx):
        return bool(self.seg_aabb(V3(*map(float, p0)), V3(*map(float, p1)), V3(*map(float, mn)), V3(*map(float, mx))))

    def shape_raycast(self, shape_type, shape_param, pos, orn, p0, p1):
        """(fraction, normal[3], feature, feature_index) as the device reports them."""
        f, T = self.fn[int(shape_type)]
        sp = [float(x) for x in shape_param]
        if shape_type == 1:
            sh = Box((C.c_float * 3)(*sp[:3]))
        elif shape_type == 2:
            sh = Sphere(sp[0])
        elif shape_type == 3:
            sh = Plane((C.c_float * 3)(*sp[:3]), sp[3])
        else:
            sh = Axial(sp[0], sp[1], int(sp[2]))
        ctx = Ctx((C.c_float * 3)(*map(float, pos)), (C.c_float * 4)(*map(float, orn)), (C.c_float * 3)(*map(float, p0)),
                  (C.c_float * 3)(*map(float, p1)))
        r = f(C.byref(sh), C.byref(ctx))
        st = bytes(r.storage)
        v = r.index
        if v in (V_BOX, V_POLYHEDRON):
            feat, idx = FEATURE_OF[(v, 0)], int.from_bytes(st[0:8], "little")
        elif v in (V_CYLINDER, V_CAPSULE):
            feat, idx = FEATURE_OF[(v, st[0])], int.from_bytes(st[8:16], "little")
        else:
            feat, idx = 0, 0
        return np.float32(r.fraction), np.array(r.normal[:], np.float32), feat, idx & 0xFFFFFFFF
