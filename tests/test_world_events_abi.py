"""Contact events and point ids on multi-device worlds at the C-ABI (edynhip_world_get_contact_events, edynhip_world_get_point_ids):
declared in include/edynhip.h, exported by the library, listed in edyn_amd._capi.SYMBOLS and bound by MultiWorld; additive (the ABI
version stays 15); a NULL world or a NULL count is EDYNHIP_ERR_INVALID before anything else is looked at. What the calls return is
tests/test_world_contact_events.py (GPU)."""
import ctypes as C
import os
import re

from edyn_amd import _capi
from edyn_amd.multi import MultiWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "edynhip.h")).read(), flags=re.S)


def test_header_declares_both_functions():
    h = _header()
    assert re.search(r"\bint\s+edynhip_world_get_contact_events\s*\(\s*edynhip_world\s*\*\s*\w+\s*,\s*edynhip_contact_event\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+edynhip_world_get_point_ids\s*\(\s*edynhip_world\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;", h)


def test_library_exports_them_and_null_world_is_invalid():
    lib = C.CDLL(_capi.LIB_PATH)
    n = C.c_uint32(7)
    buf = (C.c_uint8 * 256)()
    for name in ("edynhip_world_get_contact_events", "edynhip_world_get_point_ids"):
        f = getattr(lib, name)
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        f.restype = C.c_int
        assert f(None, None, 0, C.byref(n)) == ERR_INVALID, name
        assert f(None, C.addressof(buf), 4, C.byref(n)) == ERR_INVALID, name
        assert f(None, None, 0, None) == ERR_INVALID, name
        # n == NULL: refused before the handle is followed
        fake = (C.c_uint8 * 4096)()
        assert f(C.addressof(fake), None, 0, None) == ERR_INVALID, name


def test_binding_lists_and_wraps_them():
    L = _capi.lib()
    for name in ("edynhip_world_get_contact_events", "edynhip_world_get_point_ids"):
        assert name in _capi.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)
    assert callable(MultiWorld.get_contact_events) and callable(MultiWorld.get_point_ids)


def test_abi_version_is_unchanged():
    assert _capi.lib().edynhip_abi_version() == 15
