"""Body edits through the C++ drop-in shim (include/edyn/edyn.hpp): set_rigidbody_mass / _inertia / _friction, rigidbody_set_shape and
rigidbody_set_kind reach the running device context in place (edynhip_edit_bodies). tests/cpp/body_edits.cpp runs one program - a
4x4x4 pile, a hinge chain, a puck, ten updates between the edits - in place and with init_config::rebuild_on_body_edit: every body's
state bitwise equal after every update, no context rebuild in place, the contact entities of an untouched resting pair kept in place
and made again by the rebuild; and once more in execution_mode::asynchronous. Both registry branches."""
import os
import subprocess

import pytest
from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.gpu
@pytest.mark.parametrize("prog", ["body_edits", "body_edits_entt"])
def test_shim_body_edits_in_place(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "BODY_EDITS_OK" in out.stdout, out.stdout + out.stderr
