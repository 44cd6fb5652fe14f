"""edynhip_edit_bodies in the C-ABI, without a GPU: the symbol is exported, the field-group values are the documented ones, the ABI
version is unchanged (the entry point is additive), and a NULL context is refused before anything else is looked at."""
import ctypes as C
import os
import re

from edyn_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "edynhip.h")).read()


def test_symbol_is_exported_and_listed():
    lib = _capi.lib()
    assert hasattr(lib, "edynhip_edit_bodies")
    assert "edynhip_edit_bodies" in _capi.SYMBOLS
    assert re.search(r"int\s+edynhip_edit_bodies\s*\(\s*edynhip_ctx\s*\*\s*\w*,\s*uint32_t\s+n,\s*const\s+uint32_t\s*\*\s*indices,"
                     r"\s*const\s+edynhip_bodies\s*\*\s*values,\s*uint32_t\s+fields\s*\)", _header())


def test_field_group_values():
    want = {"EDYNHIP_EDIT_MASS": 1, "EDYNHIP_EDIT_INERTIA": 2, "EDYNHIP_EDIT_MATERIAL": 4, "EDYNHIP_EDIT_SHAPE": 8, "EDYNHIP_EDIT_KIND": 16}
    got = {k: int(v) for k, v in re.findall(r"\b(EDYNHIP_EDIT_[A-Z]+)\s*=\s*(\d+)", _header())}
    assert got == want
    assert (_capi.EDIT_MASS, _capi.EDIT_INERTIA, _capi.EDIT_MATERIAL, _capi.EDIT_SHAPE, _capi.EDIT_KIND) == (1, 2, 4, 8, 16)


def test_abi_version_stays_15():
    assert _capi.lib().edynhip_abi_version() == 15


def test_null_context_is_invalid():
    lib = _capi.lib()
    idx = (C.c_uint32 * 1)(0)
    values = _capi.Bodies()
    assert lib.edynhip_edit_bodies(None, 1, idx, C.byref(values), _capi.EDIT_MASS) == -1   # EDYNHIP_ERR_INVALID
    assert lib.edynhip_edit_bodies(None, 0, None, None, 0) == -1
