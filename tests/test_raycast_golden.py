"""The device's raycasts against the reference's own edyn::raycast: tests/golden/raycast_<kind>.npz hold what the real engine returns
for 20 000 rays of each kind (random, starting inside shapes, grazing faces and boxes, parallel to axes and faces, crossing the plane
both ways) on a scene with every shape, polyhedra and centre-of-mass offsets included (tests/golden/make_raycast.py). The device builds
the same scene in zero gravity, steps once, and must return the same body, fraction, normal, feature and index for every ray. An
exact tie in fraction may go to another body (the reference takes its tree's order, the device the lowest index): such a ray must
give the reference's body once the device's choice is ignored."""
import os
import sys

import numpy as np
import pytest

import edyn_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_raycast as mr   # noqa: E402

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
FEATURE = {(0, 0): 0, (1, 0): 1, (2, 0): 2, (2, 1): 3, (3, 0): 4, (3, 1): 5, (4, 0): 6}


@pytest.fixture(scope="module")
def world():
    s = mr.scene()
    w = edyn_amd.World(edyn_amd.init_config(gravity=(0.0, 0.0, 0.0)))
    w.set_scene(s)
    w.step_simulation(1)
    return s, w


def _same(dev, ref):
    """Per ray: the device's record equals the reference's (normals only where the reference defines one)."""
    hit = ref["entity"] != NONE
    ok = (dev["body"] == ref["entity"]) & (dev["fraction"] == ref["fraction"])
    feat = np.array([FEATURE[(int(v), int(f))] for v, f in zip(ref["variant"], ref["feature"])], np.int32)
    idx = np.where(ref["index"] < 0, np.uint32(NONE), ref["index"].astype(np.uint32))
    ok &= ~hit | ((dev["feature"] == feat) & (dev["feature_index"] == idx))
    nrm = np.all(dev["normal"] == ref["normal"], axis=1)
    ok &= ~hit | (ref["normal_defined"] == 0) | nrm
    return ok


@pytest.mark.parametrize("kind", mr.KINDS)
def test_device_equals_reference_raycast(world, kind):
    s, w = world
    p0, p1 = mr.rays(kind, s)
    fx = np.load(os.path.join(os.path.dirname(mr.__file__), f"raycast_{kind}.npz"))
    assert str(fx["rays_sha256"]) == mr.digest(p0, p1) and str(fx["scene_sha256"]) == mr.scene_digest(s)
    ref = fx["result"]
    dev = w.raycast(p0, p1)
    ok = _same(dev, ref)
    bad = np.flatnonzero(~ok)
    ties = 0
    for i in bad:   # an exact tie: with the device's choice ignored, the reference's body comes out
        if dev["fraction"][i] != ref["fraction"][i] or dev["body"][i] == NONE:
            continue
        again = w.raycast(p0[i], p1[i], ignore=[int(dev["body"][i])])
        if _same(again, ref[i:i + 1])[0]:
            ties += 1
    assert ties == len(bad), (kind, len(bad) - ties, [(int(i), dev[i], ref[i]) for i in bad[:5]])
    hit = ref["entity"] != NONE
    assert hit.sum() > 2000
    if kind in ("inside", "parallel"):
        assert (ref["variant"][hit] == 4).sum() > 1000   # polyhedra reached
