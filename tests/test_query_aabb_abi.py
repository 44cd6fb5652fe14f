"""edynhip_query_aabb / edynhip_query_aabb_device: declared in include/edynhip.h, exported by libedynhip.so, and bound by edyn_amd._capi
with the header's argument types. Needs no GPU: without one the calls fail loudly through a NULL context, as the rest of the ABI does."""
import ctypes as C
import os
import re

from conftest import ROOT

from edyn_amd import _capi

ERR_INVALID = -1   # EDYNHIP_ERR_INVALID
HEADER = os.path.join(ROOT, "include", "edynhip.h")
CTYPE = {"edynhip_ctx *": C.c_void_p, "int": C.c_int, "uint32_t": C.c_uint32, "const float *": C.c_void_p, "const void *": C.c_void_p,
         "void *": C.c_void_p, "uint32_t *": (C.c_void_p, C.POINTER(C.c_uint32)), "uint64_t *": (C.c_void_p, C.POINTER(C.c_uint64))}


def _declared(name):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name + " is not declared in edynhip.h"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        t = re.match(r"(.*?)(\w+)$", a).group(1).strip()
        args.append(t)
    return args


def test_header_declares_the_entries_and_constants():
    assert _declared("edynhip_query_aabb") == ["edynhip_ctx *", "int", "uint32_t", "const float *", "uint32_t", "uint32_t *", "uint32_t *",
                                               "uint32_t", "uint32_t *"]
    assert _declared("edynhip_query_aabb_device") == ["edynhip_ctx *", "int", "uint32_t", "const void *", "uint32_t", "void *", "void *",
                                                      "uint32_t", "void *"]
    text = open(HEADER).read()
    assert re.search(r"EDYNHIP_QUERY_PROCEDURAL = 0, EDYNHIP_QUERY_NON_PROCEDURAL = 1, EDYNHIP_QUERY_ISLANDS = 2", text)
    assert re.search(r"EDYNHIP_QUERY_BRUTE_FORCE = 1", text)
    assert (_capi.QUERY_PROCEDURAL, _capi.QUERY_NON_PROCEDURAL, _capi.QUERY_ISLANDS, _capi.QUERY_BRUTE_FORCE) == (0, 1, 2, 1)


def test_library_exports_and_capi_binds_them_with_the_headers_types():
    L = _capi.lib()
    assert L.edynhip_abi_version() == 15   # additive entries: the version stays
    for name in ("edynhip_query_aabb", "edynhip_query_aabb_device", "edynhip_query_aabb_stats"):
        assert name in _capi.SYMBOLS
        fn = getattr(L, name)   # AttributeError when libedynhip.so does not export it
        decl = _declared(name)
        assert len(fn.argtypes) == len(decl), name
        for got, t in zip(fn.argtypes, decl):
            want = CTYPE[t]
            assert got in (want if isinstance(want, tuple) else (want,)), (name, t, got)


def test_null_context_fails_loudly():
    L = _capi.lib()
    off = (C.c_uint32 * 2)()
    total = C.c_uint32(7)
    box = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert L.edynhip_query_aabb(None, 0, 1, box, 0, off, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_query_aabb_device(None, 0, 1, box, 0, off, None, 0, C.byref(total)) == ERR_INVALID
    assert L.edynhip_query_aabb_stats(None, None, None) == ERR_INVALID
