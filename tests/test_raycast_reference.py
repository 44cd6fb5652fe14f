"""The reference's own raycast routines, reached through tests/raycast_ref.py, still reproduce test/edyn/collision/test_raycast.cpp:
the helper the GPU raycast tests compare against reads the reference's result layout right (no GPU needed)."""
import numpy as np
import pytest

import raycast_ref

pytestmark = pytest.mark.skipif(not raycast_ref.available(), reason="oracle/_ref/libedynref.so is absent (built where the reference sources are)")


def test_reference_layout_reproduces_test_raycast_cpp():
    ref = raycast_ref.RefRaycast()
    box, pos, orn = (0.5, 0.5, 0.5, 0), (0.5, 0.5, 0.5), (0, 0, 0, 1)
    f, n, feat, idx = ref.shape_raycast(1, box, pos, orn, (2, 2, 2), (0, 0, 0))
    assert f == np.float32(0.5) and feat == 1
    f, n, feat, idx = ref.shape_raycast(1, box, pos, orn, (0.5, 2, 0.5), (0.5, 0, 0.5))
    assert f == np.float32(0.5) and feat == 1 and idx == 2 and np.array_equal(n, np.float32([0, 1, 0]))
    assert ref.intersect_segment_aabb((2, 2, 2), (0, 0, 0), (-0.1, -0.1, -0.1), (1.1, 1.1, 1.1))
    assert not ref.intersect_segment_aabb((2, 2, 2), (3, 3, 3), (-0.1, -0.1, -0.1), (1.1, 1.1, 1.1))


def test_reference_feature_codes_of_every_shape():
    ref = raycast_ref.RefRaycast()
    orn = (0, 0, 0, 1)
    assert ref.shape_raycast(2, (0.5, 0, 0, 0), (0, 0, 0), orn, (0, 2, 0), (0, -2, 0))[2:] == (0, 0)                  # sphere
    assert ref.shape_raycast(3, (0, 1, 0, 0), (0, 0, 0), orn, (0, 2, 0), (0, -2, 0))[0] == np.float32(0.5)          # plane
    assert ref.shape_raycast(5, (0.3, 0.5, 1, 0), (0, 0, 0), orn, (0, 2, 0.01), (0, -2, 0))[2] == 2                   # cylinder face
    assert ref.shape_raycast(5, (0.3, 0.5, 0, 0), (0, 0, 0), orn, (0, 2, 0.01), (0, -2, 0))[2] == 3                   # cylinder side edge
    assert ref.shape_raycast(4, (0.3, 0.5, 1, 0), (0, 0, 0), orn, (0, 2, 0.01), (0, -2, 0))[2:] in ((4, 0), (4, 1))    # capsule hemisphere
    assert ref.shape_raycast(4, (0.3, 0.5, 0, 0), (0, 0, 0), orn, (0, 2, 0.01), (0, -2, 0))[2] == 5                   # capsule side


def _golden():
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_raycast
    return make_raycast


@pytest.mark.parametrize("kind", ["random", "inside", "grazing", "parallel", "plane"])
def test_committed_fixtures_are_what_the_reference_returns(kind):
    """tests/golden/raycast_<kind>.npz: the reference's own edyn::raycast over the fixture's rays and scene, recomputed now."""
    import os
    mr = _golden()
    s = mr.scene()
    p0, p1 = mr.rays(kind, s)
    fx = np.load(os.path.join(os.path.dirname(mr.__file__), f"raycast_{kind}.npz"))
    assert str(fx["scene_sha256"]) == mr.scene_digest(s) and str(fx["rays_sha256"]) == mr.digest(p0, p1)
    got = mr.mark_undefined(mr.reference_raycast(mr.reference_world(s), p0, p1), s, p0, p1)
    assert np.array_equal(got, fx["result"])
    assert len(got) >= 20000 and (got["entity"] != 0xFFFFFFFF).sum() > 2000
    assert got["entity"][got["entity"] != 0xFFFFFFFF].max() < len(s["kind"])
