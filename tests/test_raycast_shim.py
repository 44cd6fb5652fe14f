"""edyn::raycast through the C++ shim (include/edyn/collision/raycast.hpp): tests/cpp/raycast.cpp on both registry branches - the
reference's test_raycast.cpp, a probe onto a resting box, the ignore list, a registry edit seen without an update, the batch overload
against single calls, and the rejection in execution_mode::asynchronous. One program at a time (one device process besides pytest)."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_shim_raycast_compiles_on_both_registry_branches():
    subprocess.check_call(["make", "-s", "-C", CPP, "raycast", "raycast_entt"])
    assert os.path.exists(os.path.join(CPP, "raycast")) and os.path.exists(os.path.join(CPP, "raycast_entt"))


@pytest.mark.gpu
@pytest.mark.parametrize("prog", ["raycast", "raycast_entt"])
def test_shim_raycast(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "RAYCAST_OK 1" in out.stdout, out.stdout + out.stderr
