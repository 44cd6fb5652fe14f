"""Materials through the C++ drop-in on a world over several devices (tests/cpp/multi_materials.cpp): edyn::attach with
init_config::devices = {0, 0}, bodies whose `material` carries contact_extras fields and ids, edyn::insert_material_mixing before the
first update and while the world runs, a body with a material made while it runs, materials changed while it runs
(edyn::refresh<edyn::material>) - the trajectory, the contact entities' data and the device's manifold records and point extras
(friction, restitution, mixed coefficients, rolling / spinning impulses) equal the same registry program on one device, bit for bit,
through at least one re-partition that carries the points' extras. Both registry branches: the bundled mini registry and <entt/entt.hpp>."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("prog", ["multi_materials", "multi_materials_entt"])
def test_materials_on_two_shards_equal_one_device(prog):
    subprocess.check_call(["make", "-s", "-C", CPP, prog])
    out = subprocess.run([os.path.join(CPP, prog)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "MULTI_MATERIALS_OK" in out.stdout, out.stdout + out.stderr
