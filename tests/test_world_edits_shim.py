"""Edits of a running multi-device world through the C++ shim (include/edyn/edyn.hpp, init_config::devices): tests/cpp/multi_edit.cpp runs
the registry program of multi_shim.cpp on one device and on two shards, makes a body and a constraint, destroys a body, changes the
gravity and kicks a body through edyn::refresh while the worlds run - and the two registries agree bit for bit at every step to step 160,
the steps after the edits included. One program at a time (one device process besides pytest)."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_multi_edit_compiles():
    subprocess.check_call(["make", "-s", "-C", CPP, "multi_edit"])
    assert os.path.exists(os.path.join(CPP, "multi_edit"))


@pytest.mark.gpu
def test_shim_forwards_edits_to_the_running_world():
    subprocess.check_call(["make", "-s", "-C", CPP, "multi_edit"])
    out = subprocess.run([os.path.join(CPP, "multi_edit")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MULTI_EDIT_OK" in out.stdout, out.stdout + out.stderr
