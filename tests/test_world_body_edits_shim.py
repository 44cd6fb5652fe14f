"""Body edits and wake_up_entity on a multi-device world through the C++ shim (include/edyn/edyn.hpp, init_config::devices):
tests/cpp/multi_body_edits.cpp runs the registry program of tests/cpp/body_edits.cpp on one device and on two shards -
set_rigidbody_mass / _inertia / _friction, rigidbody_set_shape, rigidbody_set_kind there and back, wake_up_entity with sleeping on - and the
two registries agree bit for bit after every update; the world is never rebuilt, the contact entities of an untouched resting pair stay
the same entities across every edit, and init_config::rebuild_on_body_edit makes them again. One program at a time (one device process
besides pytest)."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_multi_body_edits_compiles():
    subprocess.check_call(["make", "-s", "-C", CPP, "multi_body_edits"])
    assert os.path.exists(os.path.join(CPP, "multi_body_edits"))


@pytest.mark.gpu
def test_shim_edits_bodies_of_the_running_world_in_place():
    subprocess.check_call(["make", "-s", "-C", CPP, "multi_body_edits"])
    out = subprocess.run([os.path.join(CPP, "multi_body_edits")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MULTI_BODY_EDITS_OK" in out.stdout, out.stdout + out.stderr
