"""edyn::query_procedural_aabb / query_non_procedural_aabb through the C++ shim (include/edyn/collision/query_aabb.hpp):
tests/cpp/query_aabb.cpp on both registry branches - the forwarding header compiled on its own, the entities of a box around one body,
none after registry.destroy, the batched overload against single calls, and the rejection in execution_mode::asynchronous and on a world
over several devices. One program at a time (one device process besides pytest)."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_shim_query_aabb_compiles_on_both_registry_branches():
    subprocess.check_call(["make", "-s", "-C", CPP, "query_aabb", "query_aabb_entt"])
    assert os.path.exists(os.path.join(CPP, "query_aabb")) and os.path.exists(os.path.join(CPP, "query_aabb_entt"))


@pytest.mark.gpu
@pytest.mark.parametrize("prog", ["query_aabb", "query_aabb_entt"])
def test_shim_query_aabb(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "QUERY_AABB_OK 1" in out.stdout, out.stdout + out.stderr
