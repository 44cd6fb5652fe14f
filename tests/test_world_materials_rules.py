"""The host rules of materials on a multi-device world (edyn_amd/csrc/world_rules.hpp "materials": which materials are the default,
the 128-byte extras row of a manifold and its reading as edynhip_get_point_extras reports it, which shards a body range touches,
whether a re-partition carries point extras) - plain C++ without HIP, checked by tests/cpp/world_materials_rules.cpp against values
written from the rules' statements. No GPU needed."""
import os
import subprocess
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_world_materials_rules():
    subprocess.check_call(["make", "-s", "-C", CPP, "world_materials_rules"])
    out = subprocess.run([os.path.join(CPP, "world_materials_rules")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "WORLD_MATERIALS_RULES_OK" in out.stdout, out.stdout + out.stderr
