"""Random shape-pair batches for the closest-feature (collide) parity tests: a good share of the pairs are within the
contact threshold of each other, and degenerate SAT configurations (parallel faces / edges, equal boxes) are over-represented."""
import numpy as np
from edyn_amd import scenes


def random_quats(rng, n, snap_fraction=0.3):
    q = rng.normal(size=(n, 4)).astype(np.float32)
    # a share of exactly axis-aligned / 45-degree / 90-degree orientations: the degenerate SAT cases (parallel faces and
    # edges) are where the feature-selection branches of box_box differ most
    special = np.array([[0, 0, 0, 1], [0, 0.70710678, 0, 0.70710678], [0.38268343, 0, 0, 0.92387953],
                        [0, 0, 0.70710678, 0.70710678], [0.5, 0.5, 0.5, 0.5]], np.float32)
    pick = rng.random(n) < snap_fraction
    q[pick] = special[rng.integers(0, len(special), pick.sum())]
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    return q.astype(np.float32)


def pair_batch(rng, n, tA, tB, mesh_radii=None):
    """n shape pairs placed so that a good share are within the contact threshold of each other."""
    st = np.empty((n, 2), np.int32); st[:, 0] = tA; st[:, 1] = tB
    sp = np.zeros((n, 2, 4), np.float32)
    pos = np.zeros((n, 2, 3), np.float32)
    orn = np.stack([random_quats(rng, n), random_quats(rng, n)], axis=1)
    reach = np.zeros((n, 2), np.float32)
    for side, t in enumerate((tA, tB)):
        if t == scenes.SHAPE_BOX:
            h = rng.uniform(0.1, 0.6, size=(n, 3)).astype(np.float32)
            if side == 1:   # equal boxes in a share of the pairs (stacked-brick degeneracy)
                same = rng.random(n) < 0.3
                h[same] = sp[same, 0, :3] if tA == scenes.SHAPE_BOX else h[same]
            sp[:, side, :3] = h
            reach[:, side] = h.min(axis=1) + rng.random(n).astype(np.float32) * (np.linalg.norm(h, axis=1) - h.min(axis=1))
        elif t == scenes.SHAPE_SPHERE:
            sp[:, side, 0] = rng.uniform(0.1, 0.5, size=n)
            reach[:, side] = sp[:, side, 0]
        elif t == getattr(scenes, "SHAPE_CAPSULE", 4):   # (radius, half_length, axis)
            sp[:, side, 0] = rng.uniform(0.1, 0.4, size=n)
            sp[:, side, 1] = rng.uniform(0.05, 0.6, size=n)
            sp[:, side, 2] = rng.integers(0, 3, n)
            reach[:, side] = sp[:, side, 0] + rng.random(n).astype(np.float32) * sp[:, side, 1]
        elif t == getattr(scenes, "SHAPE_CYLINDER", 5):   # (radius, half_length, axis): flat discs and long rods alike
            sp[:, side, 0] = rng.uniform(0.1, 0.5, size=n)
            sp[:, side, 1] = rng.uniform(0.05, 0.6, size=n)
            sp[:, side, 2] = rng.integers(0, 3, n)
            r, hl = sp[:, side, 0], sp[:, side, 1]
            reach[:, side] = np.minimum(r, hl) + rng.random(n).astype(np.float32) * (np.sqrt(r * r + hl * hl) - np.minimum(r, hl))
        elif t == getattr(scenes, "SHAPE_POLYHEDRON", 6):   # shape_param[0] = mesh id; mesh_radii[id] = (inner, outer) about the centroid
            ids = rng.integers(0, len(mesh_radii), n)
            sp[:, side, 0] = ids
            rr = np.asarray(mesh_radii, np.float32)[ids]
            reach[:, side] = rr[:, 0] + rng.random(n).astype(np.float32) ** 2 * (rr[:, 1] - rr[:, 0])
        else:   # plane through a random offset with a random (or +Y) normal
            nrm = rng.normal(size=(n, 3)).astype(np.float32)
            nrm[rng.random(n) < 0.5] = (0, 1, 0)
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
            sp[:, side, :3] = nrm
            sp[:, side, 3] = rng.uniform(-0.5, 0.5, size=n)
            orn[:, side] = (0, 0, 0, 1)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    snap = rng.random(n) < 0.4
    axes = np.eye(3, dtype=np.float32)[rng.integers(0, 3, n)] * rng.choice(np.float32([-1, 1]), size=(n, 1))
    d[snap] = axes[snap]
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    gap = rng.uniform(-0.08, 0.04, size=n).astype(np.float32)
    pos[:, 0] = rng.uniform(-2, 2, size=(n, 3))
    if tB == scenes.SHAPE_PLANE:
        pos[:, 1] = 0
        nrm = sp[:, 1, :3]
        pos[:, 0] = nrm * (sp[:, 1, 3:4] + reach[:, 0:1] + gap[:, None]) + np.cross(nrm, d) * 2
    elif tA == scenes.SHAPE_PLANE:
        pos[:, 0] = 0
        nrm = sp[:, 0, :3]
        pos[:, 1] = nrm * (sp[:, 0, 3:4] + reach[:, 1:2] + gap[:, None]) + np.cross(nrm, d) * 2
    else:
        pos[:, 1] = pos[:, 0] + d * (reach[:, 0] + reach[:, 1] + gap)[:, None]
    return st, sp, pos.astype(np.float32), orn.astype(np.float32)


EDGE_CLASSES = ("coincident", "deep", "far", "scale", "aspect", "lattice")
LATTICE_THRESHOLDS = (0.02, 0.25)   # at 0.25 a grid separation can equal the threshold exactly


def edge_pair_batch(rng, n, tA, tB, cls, mesh_radii=None):
    """pair_batch, then rewritten into one class of degenerate input (the same four arrays, float32 / int32):
      coincident  both centres in one point (with a plane: the other body's centre in the plane's own point normal * offset);
      deep        the second centre pulled towards the first by a uniform share (with a plane: the body pushed up to 1.5 below it);
      far         both bodies moved by k * (1, 1, 1), k one of 1e3, 1e4, -3e3 (a plane's offset follows): an ulp of 1e-4 .. 1e-3;
      scale       every length - extents, radii, half lengths, plane offset, positions - times 0.01 or 100 (not for polyhedra);
      aspect      plates and needles: one half extent of a box 0.004 or 5, the half length of a capsule / cylinder 0.002 or 5
                  (never 0: a capsule or cylinder without length is outside the reference's domain, oracle/README.md);
      lattice     identity orientations, sizes and positions on a 0.25 grid, the plane y = 0: exact zeros of either sign and
                  separations that equal a threshold of 0.25 exactly."""
    CAP, CYL, POLY = getattr(scenes, "SHAPE_CAPSULE", 4), getattr(scenes, "SHAPE_CYLINDER", 5), getattr(scenes, "SHAPE_POLYHEDRON", 6)
    st, sp, pos, orn = pair_batch(rng, n, tA, tB, mesh_radii)
    types = (tA, tB)
    plane = 0 if tA == scenes.SHAPE_PLANE else (1 if tB == scenes.SHAPE_PLANE else None)
    body = None if plane is None else 1 - plane
    if cls == "coincident":
        if plane is None:
            pos[:, 1] = pos[:, 0]
        else:
            pos[:, body] = sp[:, plane, :3] * sp[:, plane, 3:4]
    elif cls == "deep":
        if plane is None:
            u = rng.random(n).astype(np.float32)
            pos[:, 1] = pos[:, 0] + (pos[:, 1] - pos[:, 0]) * u[:, None]
        else:
            u = rng.uniform(0, 1.5, size=n).astype(np.float32)
            pos[:, body] = pos[:, body] - sp[:, plane, :3] * u[:, None]
    elif cls == "far":
        k = rng.choice(np.float32([1e3, 1e4, -3e3]), size=n)
        off = k[:, None] * np.ones(3, np.float32)
        if plane is None:
            pos[:, 0] += off; pos[:, 1] += off
        else:
            sp[:, plane, 3] += (sp[:, plane, :3] * off).sum(axis=1, dtype=np.float32)
            pos[:, body] += off
    elif cls == "scale":
        assert POLY not in types, "a mesh has one size"
        f = rng.choice(np.float32([0.01, 100]), size=n)
        for side, t in enumerate(types):
            if t == scenes.SHAPE_BOX:
                sp[:, side, :3] *= f[:, None]
            elif t == scenes.SHAPE_SPHERE:
                sp[:, side, 0] *= f
            elif t in (CAP, CYL):
                sp[:, side, :2] *= f[:, None]
            else:
                sp[:, side, 3] *= f
        pos *= f[:, None, None]
    elif cls == "aspect":
        for side, t in enumerate(types):
            if t == scenes.SHAPE_BOX:
                sp[np.arange(n), side, rng.integers(0, 3, n)] = rng.choice(np.float32([0.004, 5.0]), size=n)
            elif t in (CAP, CYL):
                sp[:, side, 1] = rng.choice(np.float32([0.002, 5.0]), size=n)
    elif cls == "lattice":
        orn[:] = (0, 0, 0, 1)
        for side, t in enumerate(types):
            if t == scenes.SHAPE_BOX:
                sp[:, side, :3] = rng.choice(np.float32([0.25, 0.5, 1]), size=(n, 3))
            elif t == scenes.SHAPE_SPHERE:
                sp[:, side, 0] = rng.choice(np.float32([0.25, 0.5]), size=n)
            elif t in (CAP, CYL):
                sp[:, side, :2] = rng.choice(np.float32([0.25, 0.5]), size=(n, 2))
            elif t == scenes.SHAPE_PLANE:
                sp[:, side] = (0, 1, 0, 0)
        # a mesh is smaller than the biggest grid shapes and has no size to draw: offsets of up to 6 cells leave under a tenth
        # of the pairs with a polyhedron touching, 3 cells leave more than a fifth
        reach = 3 if POLY in types else 6
        pos[:, 0] = rng.integers(-4, 5, size=(n, 3)) * np.float32(0.25)
        pos[:, 1] = pos[:, 0] + rng.integers(-reach, reach + 1, size=(n, 3)) * np.float32(0.25)
        if plane is not None:
            pos[:, plane] = 0
    else:
        raise ValueError(cls)
    return st, sp.astype(np.float32), pos.astype(np.float32), orn.astype(np.float32)
