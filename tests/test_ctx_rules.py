"""The host rules of the single-context C-ABI (edyn_amd/csrc/ctx_rules.hpp: the joints' edge colouring and colour-sorted packing, the
row count per joint type, the hinge's tangent frame, a body's exclusion list, the default should_collide, the canonical pair key and
its sortedness check, the broadphase participants) - plain C++ without HIP, checked by tests/cpp/ctx_rules.cpp against values written
from the rules' statements. No GPU and no library needed."""
import os
import subprocess
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_ctx_rules():
    subprocess.check_call(["make", "-s", "-C", CPP, "ctx_rules"])
    out = subprocess.run([os.path.join(CPP, "ctx_rules")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "CTX_RULES_OK" in out.stdout, out.stdout + out.stderr
