"""The host rules of the multi-device world (edyn_amd/csrc/world_rules.hpp: sticky targets, the rebalance trigger, the placement of
new bodies, who holds and reports a body, a joint's and an exclusion's home, bounding radii, the host island estimate, the welding
and the spatial partitioner) - plain C++ without HIP, checked by tests/cpp/world_rules.cpp against values written from the rules'
statements. No GPU and no library needed."""
import os
import subprocess
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_world_rules():
    subprocess.check_call(["make", "-s", "-C", CPP, "world_rules"])
    out = subprocess.run([os.path.join(CPP, "world_rules")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "WORLD_RULES_OK" in out.stdout, out.stdout + out.stderr
