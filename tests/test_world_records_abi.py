"""Record hand-over of a multi-device world at the C-ABI and in Python, without a GPU: edynhip_world_snapshot_records /
edynhip_world_snapshot_map are declared, exported and listed; the ABI version did not move; NULL arguments are refused; MultiWorld
has the two methods."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("edynhip_world_snapshot_records", "edynhip_world_snapshot_map")
ERR_INVALID = -1


def _header():
    txt = open(os.path.join(ROOT, "include", "edynhip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_declared_exported_and_listed():
    from edyn_amd import _capi
    declared = set(re.findall(r"\b(edynhip_[a-z_]+)\s*\(", _header()))
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
        assert not re.search(r"\d", name)
    assert lib.edynhip_abi_version() == 15


def test_signatures_in_the_header():
    h = _header()
    assert re.search(r"int\s+edynhip_world_snapshot_records\s*\(\s*edynhip_world\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*\)\s*;", h)
    assert re.search(r"int\s+edynhip_world_snapshot_map\s*\(\s*edynhip_world\s*\*\s*\w+\s*,\s*edynhip_record_view\s*\*\s*\w+\s*\)\s*;", h)


def test_null_arguments_are_invalid():
    from edyn_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    lib.edynhip_world_snapshot_records.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32]
    lib.edynhip_world_snapshot_map.argtypes = [C.c_void_p, C.c_void_p]
    view = _capi.RecordView()
    assert lib.edynhip_world_snapshot_records(None, 0.0, 16, 0) == ERR_INVALID
    assert lib.edynhip_world_snapshot_records(None, 0.0, 16, 1) == ERR_INVALID
    assert lib.edynhip_world_snapshot_map(None, C.byref(view)) == ERR_INVALID
    assert lib.edynhip_world_snapshot_map(None, None) == ERR_INVALID


def test_multiworld_has_the_methods():
    from edyn_amd.multi import MultiWorld
    assert callable(getattr(MultiWorld, "snapshot_records", None))
    assert callable(getattr(MultiWorld, "snapshot_map", None))
    import inspect
    sig = inspect.signature(MultiWorld.snapshot_records)
    assert sig.parameters["present_dt"].default == 0.0 and sig.parameters["max_events"].default == 4096
