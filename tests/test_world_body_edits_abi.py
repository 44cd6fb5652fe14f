"""edynhip_world_edit_bodies / edynhip_world_wake_bodies at the C-ABI: declared in include/edynhip.h with the signatures of
edynhip_edit_bodies / edynhip_wake_bodies on a world, exported by the library, listed in edyn_amd._capi.SYMBOLS with argument types,
bound by MultiWorld with World.edit_bodies' signature; additive (the ABI version stays at 15). Runs without a device: a NULL world is an
argument error before anything touches a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

import edyn_amd
from edyn_amd import _capi
from edyn_amd.multi import MultiWorld

ERR_INVALID = -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "edynhip.h")
SIGNATURES = {
    "edynhip_world_edit_bodies": r"int\s+edynhip_world_edit_bodies\s*\(\s*edynhip_world\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,"
                                 r"\s*const\s+edynhip_bodies\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;",
    "edynhip_world_wake_bodies": r"int\s+edynhip_world_wake_bodies\s*\(\s*edynhip_world\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*\)\s*;",
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_typed(name):
    with open(HEADER) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(SIGNATURES[name], h), name
    assert name in _capi.SYMBOLS and len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)
    fn = getattr(_capi.lib(), name)            # AttributeError: the library does not export it
    assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p, name
    single = getattr(_capi.lib(), name.replace("_world", ""))
    assert list(fn.argtypes) == list(single.argtypes), "same arguments as on one context"


def test_null_world_is_an_argument_error():
    L = _capi.lib()
    b = _capi.Bodies()
    idx = (C.c_uint32 * 1)(0)
    assert L.edynhip_world_edit_bodies(None, 1, idx, C.byref(b), _capi.EDIT_MASS) == ERR_INVALID
    assert L.edynhip_world_edit_bodies(None, 0, None, None, 0) == ERR_INVALID
    assert L.edynhip_world_wake_bodies(None, 1, idx) == ERR_INVALID
    assert L.edynhip_world_wake_bodies(None, 0, None) == ERR_INVALID


def test_additive_to_abi_15():
    assert _capi.lib().edynhip_abi_version() == 15
    assert (_capi.EDIT_MASS, _capi.EDIT_INERTIA, _capi.EDIT_MATERIAL, _capi.EDIT_SHAPE, _capi.EDIT_KIND) == (1, 2, 4, 8, 16)


def test_multiworld_binds_them_like_world():
    assert callable(MultiWorld.wake_bodies)
    a, b = inspect.signature(MultiWorld.edit_bodies), inspect.signature(edyn_amd.World.edit_bodies)
    assert [(p.name, p.default) for p in a.parameters.values()] == [(p.name, p.default) for p in b.parameters.values()]
    assert list(inspect.signature(MultiWorld.wake_bodies).parameters) == list(inspect.signature(edyn_amd.World.wake_bodies).parameters)
