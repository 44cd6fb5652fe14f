"""Raycast and AABB queries on multi-device worlds at the C-ABI (edynhip_world_raycast[_device], edynhip_world_query_aabb[_device]):
the entries are declared in include/edynhip.h, exported by the library and listed in edyn_amd._capi.SYMBOLS; they are additive (the
ABI version stays 15); arguments are validated before the world is touched, so a NULL world or NULL arrays give EDYNHIP_ERR_INVALID
without a device. What the queries return is tests/test_world_queries.py (GPU)."""
import ctypes as C
import os
import re

from edyn_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("edynhip_world_raycast", "edynhip_world_raycast_device", "edynhip_world_query_aabb", "edynhip_world_query_aabb_device")
ERR_INVALID = -1


def test_symbols_are_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "edynhip.h")).read()
    L = _capi.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*edynhip_world\s*\*", header), name
        assert name in _capi.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)


def test_abi_version_is_unchanged():
    assert _capi.lib().edynhip_abi_version() == 15


def test_null_world_and_null_arrays_are_invalid():
    L = _capi.lib()
    buf = (C.c_float * 64)()
    out = (C.c_uint8 * 256)()
    tot = C.c_uint32(0)
    p, o = C.addressof(buf), C.addressof(out)
    assert L.edynhip_world_raycast(None, 1, p, p, 0, None, 0, o) == ERR_INVALID
    assert L.edynhip_world_raycast_device(None, 1, p, p, 0, None, 0, o) == ERR_INVALID
    assert L.edynhip_world_query_aabb(None, 0, 1, p, 0, o, None, 0, C.byref(tot)) == ERR_INVALID
    assert L.edynhip_world_query_aabb_device(None, 0, 1, p, 0, o, None, 0, o) == ERR_INVALID
    # NULL arrays: refused before anything of the world is read (the handle is never followed)
    fake = (C.c_uint8 * 4096)()
    w = C.addressof(fake)
    for f in (L.edynhip_world_raycast, L.edynhip_world_raycast_device):
        assert f(w, 1, None, p, 0, None, 0, o) == ERR_INVALID
        assert f(w, 1, p, None, 0, None, 0, o) == ERR_INVALID
        assert f(w, 1, p, p, 0, None, 0, None) == ERR_INVALID
        assert f(w, 1, p, p, 2, None, 0, o) == ERR_INVALID
    assert L.edynhip_world_query_aabb(w, 0, 1, None, 0, o, None, 0, C.byref(tot)) == ERR_INVALID
    assert L.edynhip_world_query_aabb(w, 0, 1, p, 0, None, None, 0, C.byref(tot)) == ERR_INVALID
    assert L.edynhip_world_query_aabb(w, 0, 1, p, 0, o, None, 0, None) == ERR_INVALID
    assert L.edynhip_world_query_aabb_device(w, 0, 1, None, 0, o, None, 0, o) == ERR_INVALID
    assert L.edynhip_world_query_aabb_device(w, 0, 1, p, 0, None, None, 0, o) == ERR_INVALID
    assert L.edynhip_world_query_aabb_device(w, 0, 1, p, 0, o, None, 0, None) == ERR_INVALID
