"""Edits of a running multi-device world at the C-ABI (edynhip_world_add_bodies ... edynhip_world_get_edit_stats): declared in
include/edynhip.h, exported by the library, listed in edyn_amd._capi.SYMBOLS with argument types, bound by MultiWorld; additive (the ABI
version stays at 15). Runs without a device: a NULL world is an argument error before anything touches a GPU."""
import ctypes as C
import os
import re

import pytest

from edyn_amd import _capi
from edyn_amd.multi import MultiWorld

ERR_INVALID = -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "edynhip.h")
NEW = ["edynhip_world_add_bodies", "edynhip_world_remove_bodies", "edynhip_world_add_joints", "edynhip_world_remove_joints",
       "edynhip_world_edit_joint", "edynhip_world_edit_exclusion", "edynhip_world_set_state", "edynhip_world_get_params",
       "edynhip_world_set_params", "edynhip_world_get_edit_stats", "edynhip_world_get_asleep"]


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_typed(name):
    with open(HEADER) as f:
        h = f.read()
    assert re.search(r"\bint\s+%s\s*\(\s*edynhip_world\s*\*" % name, h), name
    assert name in _capi.SYMBOLS and len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)
    fn = getattr(_capi.lib(), name)            # AttributeError: the library does not export it
    assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p, name


def test_null_world_is_an_argument_error():
    L = _capi.lib()
    b, j, p, st = _capi.Bodies(), _capi.Joints(), _capi.Params(), _capi.WorldEditStats()
    first = C.c_uint32(0)
    idx = (C.c_uint32 * 1)(0)
    f = (C.c_float * 60)()
    assert L.edynhip_world_add_bodies(None, 1, C.byref(b), C.byref(first)) == ERR_INVALID
    assert L.edynhip_world_remove_bodies(None, 1, idx) == ERR_INVALID
    assert L.edynhip_world_add_joints(None, 1, C.byref(j), C.byref(first)) == ERR_INVALID
    assert L.edynhip_world_remove_joints(None, 1, idx) == ERR_INVALID
    assert L.edynhip_world_edit_joint(None, 0, f, f, f, 0) == ERR_INVALID
    assert L.edynhip_world_edit_exclusion(None, 0, 1, 1) == ERR_INVALID
    assert L.edynhip_world_set_state(None, f, f, f, f) == ERR_INVALID
    assert L.edynhip_world_get_params(None, C.byref(p)) == ERR_INVALID
    assert L.edynhip_world_set_params(None, C.byref(p)) == ERR_INVALID
    assert L.edynhip_world_get_edit_stats(None, C.byref(st)) == ERR_INVALID
    assert L.edynhip_world_get_asleep(None, f) == ERR_INVALID


def test_edit_stats_layout_and_version():
    with open(HEADER) as f:
        h = f.read()
    m = re.search(r"typedef struct \{([^}]*)\}\s*edynhip_world_edit_stats;", h)
    assert m, "edynhip_world_edit_stats is not declared"
    fields = re.findall(r"uint32_t\s+(\w+);", m.group(1))
    assert fields == [n for n, _ in _capi.WorldEditStats._fields_]
    assert C.sizeof(_capi.WorldEditStats) == 4 * len(fields) == 20
    assert _capi.lib().edynhip_abi_version() == 15            # additive: nothing an older caller uses has moved


def test_multiworld_binds_the_edits():
    for name in ("add_scene", "remove_bodies", "add_joints", "remove_joints", "set_joint_params", "set_joint_definition",
                 "set_generic_definition", "exclude_collision", "remove_collision_exclusion", "set_state", "set_params", "get_params",
                 "get_edit_stats", "get_asleep"):
        assert callable(getattr(MultiWorld, name)), name
