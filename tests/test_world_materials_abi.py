"""Materials on a multi-device world at the C-ABI (edynhip_world_set_material_extras / _set_material_ids / _insert_material_mixing /
_get_point_extras): declared in include/edynhip.h with the single-context calls' argument lists, exported by the library, listed in
edyn_amd._capi.SYMBOLS with argument types, bound by MultiWorld; additive (the ABI version stays at 15), with one counter appended to
edynhip_world_stats. Runs without a device: a NULL world is an argument error before anything touches a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

from edyn_amd import _capi
from edyn_amd.multi import MultiWorld
from edyn_amd.world import World

ERR_INVALID = -1
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "edynhip.h")
NEW = {"edynhip_world_set_material_extras": "edynhip_set_material_extras", "edynhip_world_set_material_ids": "edynhip_set_material_ids",
       "edynhip_world_insert_material_mixing": "edynhip_insert_material_mixing", "edynhip_world_get_point_extras": "edynhip_get_point_extras"}


def _header():
    with open(HEADER) as f:
        return f.read()


def _c_arguments(h, name):
    """The argument types of a declaration in the header, names and spaces dropped."""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, h)
    assert m, name + " is not declared"
    return [re.sub(r"\s+", " ", re.sub(r"\w+\s*$", "", a.strip())).strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_exported_and_typed(name):
    h = _header()
    world, single = _c_arguments(h, name), _c_arguments(h, NEW[name])
    assert world[0] == "edynhip_world *" and single[0] == "edynhip_ctx *"
    assert world[1:] == single[1:], (world, single)          # the single-context call's arguments, in its order
    assert name in _capi.SYMBOLS and len(set(_capi.SYMBOLS)) == len(_capi.SYMBOLS)
    fn, one = getattr(_capi.lib(), name), getattr(_capi.lib(), NEW[name])     # AttributeError: the library does not export it
    assert fn.argtypes is not None and len(fn.argtypes) == len(world) and list(fn.argtypes) == list(one.argtypes), name


def test_null_world_is_an_argument_error():
    L = _capi.lib()
    f = (C.c_float * 28)()
    ids = (C.c_uint32 * 1)(0)
    n = C.c_uint32(0)
    assert L.edynhip_world_set_material_extras(None, 0, 1, f, f, f, f) == ERR_INVALID
    assert L.edynhip_world_set_material_ids(None, 0, 1, ids) == ERR_INVALID
    assert L.edynhip_world_insert_material_mixing(None, 0, 1, f) == ERR_INVALID
    assert L.edynhip_world_get_point_extras(None, f, 1, C.byref(n)) == ERR_INVALID


def test_world_stats_layout_and_version():
    h = _header()
    end = h.find("} edynhip_world_stats;")
    assert end > 0, "edynhip_world_stats is not declared"
    body = re.sub(r"/\*.*?\*/", "", h[h.rfind("typedef struct {", 0, end):end], flags=re.S)
    fields = [x.strip() for decl in re.findall(r"uint32_t\s+([^;]+);", body) for x in decl.split(",")]
    names = [re.sub(r"\[\d+\]", "", x) for x in fields]
    assert names == [n for n, _ in _capi.WorldStats._fields_]
    assert names[-1] == "extras_carries" and names[-2] == "rebalances"     # appended: no earlier field has moved
    words = sum(int(re.search(r"\[(\d+)\]", x).group(1)) if "[" in x else 1 for x in fields)
    assert C.sizeof(_capi.WorldStats) == 4 * words == 92
    assert _capi.WorldStats.extras_carries.offset == 88 and _capi.WorldStats.rebalances.offset == 84
    assert C.sizeof(_capi.WorldEditStats) == 20                            # untouched
    assert _capi.lib().edynhip_abi_version() == 15                         # additive: nothing an older caller uses has moved


def test_multiworld_binds_the_calls_with_worlds_signatures():
    for name in ("set_material_extras", "set_material_ids", "insert_material_mixing", "get_point_extras"):
        assert callable(getattr(MultiWorld, name)), name
        assert inspect.signature(getattr(MultiWorld, name)) == inspect.signature(getattr(World, name)), name
