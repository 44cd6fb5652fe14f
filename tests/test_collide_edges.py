"""The closest-feature routines on DEGENERATE pairs, pair by pair: the device's (dcollide.hpp, dcylinder.hpp, dpolyhedron.hpp, through
edynhip_debug_collide) against the oracle's, and the oracle's against the real engine's.

The random-pair tests (test_gpu_parity.py, test_reference_engine.py) draw from one distribution - sizes 0.1-0.6 within +-2 of the origin,
gaps of a few centimetres. The classes of pairgen.edge_pair_batch are what that distribution never shows a routine: coincident centres, a
centre deep inside the other shape, coordinates of 1e3-1e4, shapes 100 times bigger or smaller, plates and needles, and grid poses whose
results are exact zeros of either sign and whose separations equal the threshold. Zero signs and NaN are where a min / max / clamp spelt
with the hardware instruction and one spelt with a comparison part ways, and every comparison here is on the bit patterns.

Three legs:
  * device against oracle (gpu): every class x combination, then mixed batches at the sizes where edynhip_debug_collide's kernel
    selection, the polyhedron kernel's slicing and a half-empty last wavefront can go wrong;
  * oracle against the real engine (CPU; skipped where oracle/_ref was not built): the same batches - the oracle is a specification
    on these inputs only as far as this leg holds;
  * what the batches must contain, asserted on the oracle's output alone (CPU, no engine needed): so that no leg passes on empty input.
"""
import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from oracle import binding as ob
from pairgen import EDGE_CLASSES, LATTICE_THRESHOLDS, edge_pair_batch, pair_batch
import meshes

B, S, PL, C, CY, P = (scenes.SHAPE_BOX, scenes.SHAPE_SPHERE, scenes.SHAPE_PLANE, scenes.SHAPE_CAPSULE, scenes.SHAPE_CYLINDER,
                      scenes.SHAPE_POLYHEDRON)
# the 24 ordered combinations of test_collide_routines_bit_exact_on_random_pairs, and the polyhedron's six partners
COMBOS = [(B, B), (S, B), (B, S), (S, S), (B, PL), (PL, B), (S, PL), (PL, S), (C, C), (C, B), (B, C), (C, S), (S, C), (C, PL), (PL, C),
          (CY, PL), (PL, CY), (CY, S), (S, CY), (CY, CY), (CY, B), (B, CY), (C, CY), (CY, C)]
POLY_PARTNERS = [PL, S, P, B, C, CY]
NAMES = {B: "box", S: "sphere", PL: "plane", C: "capsule", CY: "cylinder", P: "polyhedron"}
N_PLAIN, N_POLY = 20_000, 5_000
MAX_NON_FINITE = 0.01     # share of pairs with a non-finite value in the oracle's used slots
MIN_TOUCHING = 0.05       # share of pairs with at least one point
# (class, threshold) cases: the grid class also at a threshold that is itself on the grid
CASES = [(cls, thr) for cls in EDGE_CLASSES for thr in (LATTICE_THRESHOLDS if cls == "lattice" else (0.02,))]
CASES_POLY = [c for c in CASES if c[0] != "scale"]


def _case_id(case):
    return case[0] if case[0] != "lattice" else f"lattice-thr{case[1]}"


def _orders(other):
    return ((P, other), (other, P)) if other != P else ((P, P),)


def _batch(cls, tA, tB):
    """The pairs of one (class, combination): the seed is a function of the three alone, every leg sees the same pairs."""
    _, rad = meshes.registered()
    poly = P in (tA, tB)
    rng = np.random.default_rng(5000 + 100 * EDGE_CLASSES.index(cls) + 10 * tA + tB)
    return edge_pair_batch(rng, N_POLY if poly else N_PLAIN, tA, tB, cls, rad if poly else None)


def _used(cnt):
    return np.arange(4)[None, :] < cnt[:, None]


def _assert_caps(op, oc, what):
    """What a batch must contain, on the oracle's arrays only. Returns the per-pair 'finite' mask."""
    used = _used(oc)
    finite = ~(used[:, :, None] & ~np.isfinite(op)).any(axis=(1, 2))
    share_nf, share_touch = 1.0 - finite.mean(), (oc > 0).mean()
    print(f"[edges] {what}: non-finite pairs {share_nf:.4%}, touching {share_touch:.2%}")
    assert share_nf <= MAX_NON_FINITE, (what, share_nf)
    assert share_touch >= MIN_TOUCHING, (what, share_touch)
    return finite


def _assert_device_matches(gp, gc, op, oc, what):
    """Counts equal; on pairs whose oracle values are all finite the used slots bit for bit; on the others the same values are NaN
    (sign and payload of a NaN are not part of the specification) and every other value, infinities included, bit for bit."""
    assert np.array_equal(gc, oc), (what, "counts", np.flatnonzero(gc != oc)[:8])
    finite = _assert_caps(op, oc, what)
    used = _used(oc)
    g, o = gp[used], op[used]                                # [points, 11]
    fin = np.repeat(finite, oc.astype(np.int64))             # the pair each used point belongs to (row-major, like the mask)
    gb, obits = g.view(np.uint32), o.view(np.uint32)
    bad = np.flatnonzero((gb[fin] != obits[fin]).any(axis=1))
    assert bad.size == 0, (what, "bits differ on finite pairs", bad.size, g[fin][bad[:4]], o[fin][bad[:4]])
    if not fin.all():
        gn, on = np.isnan(g[~fin]), np.isnan(o[~fin])
        assert np.array_equal(~np.isfinite(g[~fin]), ~np.isfinite(o[~fin])), (what, "non-finite masks differ")
        assert np.array_equal(gn, on), (what, "NaN masks differ")
        assert np.array_equal(gb[~fin][~on], obits[~fin][~on]), (what, "bits differ beside the NaNs")


# ------------------------------------------------------------------------------------------- device against oracle
@pytest.fixture(scope="module")
def world():
    lib, _ = meshes.registered()
    w = edyn_amd.World(edyn_amd.init_config())
    for k, m in enumerate(lib):
        assert w.create_convex_mesh(m["vertices"], m["indices"], m["faces"]) == k
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("tA,tB", COMBOS, ids=lambda t: NAMES[t])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_device_collide_bit_exact_on_degenerate_pairs(world, case, tA, tB):
    """20k pairs of one class per combination through the device routines and the oracle's: counts, pivots, normals, distances and
    attachments bit for bit, zero signs included; where the oracle's own result is not finite, the same values are."""
    cls, thr = case
    st, sp, pos, orn = _batch(cls, tA, tB)
    gp, gc = world.debug_collide(st, sp, pos, orn, threshold=thr)
    op, oc = ob.collide_batch(st, sp, pos, orn, threshold=thr)
    _assert_device_matches(gp, gc, op, oc, f"{_case_id(case)} {NAMES[tA]}-{NAMES[tB]}")


@pytest.mark.gpu
@pytest.mark.parametrize("other", POLY_PARTNERS, ids=lambda t: NAMES[t])
@pytest.mark.parametrize("case", CASES_POLY, ids=_case_id)
def test_device_polyhedron_collide_bit_exact_on_degenerate_pairs(world, case, other):
    """5k pairs per class and argument order over the ten meshes of tests/meshes.py. The pairs of polyhedra on which the reference is
    undefined (ob.last_batch_flags) stay in: there the oracle's definition is the device's specification."""
    cls, thr = case
    for tA, tB in _orders(other):
        st, sp, pos, orn = _batch(cls, tA, tB)
        gp, gc = world.debug_collide(st, sp, pos, orn, threshold=thr)
        op, oc = ob.collide_batch(st, sp, pos, orn, threshold=thr)
        _assert_device_matches(gp, gc, op, oc, f"{_case_id(case)} {NAMES[tA]}-{NAMES[tB]}")


# ---- edynhip_debug_collide's own dispatch: what a batch of one combination never mixes
ALL_COMBOS = COMBOS + [o for other in POLY_PARTNERS for o in _orders(other)]


def _mixed_batch(seed, n, combos, last=None):
    """n pairs, each pair's combination drawn independently from `combos`, from the ordinary pair_batch distribution: assembled per
    combination, then shuffled. `last`: one more pair of that combination appended after the shuffle."""
    _, rad = meshes.registered()
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(combos), n)
    parts = [pair_batch(rng, int((pick == k).sum()), tA, tB, rad) for k, (tA, tB) in enumerate(combos) if (pick == k).any()]
    perm = rng.permutation(n)
    arrays = [np.concatenate([p[f] for p in parts])[perm] for f in range(4)]
    if last is not None:
        tail = pair_batch(rng, 1, last[0], last[1], rad)
        arrays = [np.concatenate([a, t]) for a, t in zip(arrays, tail)]
    return arrays


# seeds: fixed; the one of the single-pair batch is one whose pair touches (the share of touching pairs of one pair is 0 or 1)
MIXED = [("n1", 5, 1, ALL_COMBOS, None), ("n63", 11, 63, ALL_COMBOS, None), ("n64", 12, 64, ALL_COMBOS, None), ("n65", 13, 65, ALL_COMBOS, None),
         ("n4099", 14, 4099, ALL_COMBOS, None), ("one_polyhedron_pair_last", 15, 129, COMBOS, (P, B))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,combos,last", MIXED, ids=[m[0] for m in MIXED])
def test_device_collide_dispatch_on_mixed_batches(world, name, seed, n, combos, last):
    """One batch with every ordered combination in it, polyhedra included, in random order: the plain kernel, the cylinder kernel
    (k_debug_collide<EXT>) and the polyhedron kernel each have to find their own pairs and leave the others' results alone. Sizes of one
    pair, one short of / exactly / one over a 64-lane block, and 4099 (65 blocks, a last block of three lanes); and a batch whose only
    polyhedron pair is its last element, the polyhedron kernel's last slice and block."""
    st, sp, pos, orn = _mixed_batch(seed, n, combos, last)
    assert len(st) == n + (last is not None)
    if last is not None:
        assert (st[:-1] != P).all() and tuple(st[-1]) == last
    elif n >= 4099:
        assert len({tuple(x) for x in st}) == len(ALL_COMBOS)
    gp, gc = world.debug_collide(st, sp, pos, orn, threshold=0.02)
    op, oc = ob.collide_batch(st, sp, pos, orn, threshold=0.02)
    _assert_device_matches(gp, gc, op, oc, f"mixed {name}")


# ------------------------------------------------------------------------------------------- what the batches must contain
def test_lattice_batches_hold_negative_zeros_and_separations_equal_to_the_threshold():
    """The grid class is there for two things, and has to deliver them (oracle's output only): a -0.0 (0x80000000) among the values of
    the used slots, and at a threshold of 0.25 a point whose distance IS the threshold. Both over the class as a whole."""
    neg_zero = at_threshold = 0
    for tA, tB in ALL_COMBOS:
        st, sp, pos, orn = _batch("lattice", tA, tB)
        for thr in LATTICE_THRESHOLDS:
            op, oc = ob.collide_batch(st, sp, pos, orn, threshold=thr)
            pts = op[_used(oc)]
            neg_zero += int((pts.view(np.uint32) == 0x80000000).any(axis=1).sum())
            if thr == 0.25:
                at_threshold += int((pts[:, 9] == np.float32(0.25)).sum())
    print(f"[edges] lattice: {neg_zero} points with a -0.0, {at_threshold} points at distance == threshold")
    assert neg_zero > 0 and at_threshold > 0


# ------------------------------------------------------------------------------------------- oracle against the real engine
needs_engine = pytest.mark.skipif(ob.ref() is None, reason="oracle/_ref/libedynref.so not built (needs the reference's source at build time)")
MAX_FLAGGED = 0.02           # polyhedron pairs on which the reference is undefined, outside the grid class
MAX_FLAGGED_LATTICE = 0.40   # ... and on the grid


def _assert_oracle_matches_engine(cls, thr, tA, tB):
    st, sp, pos, orn = _batch(cls, tA, tB)
    what = f"{cls} thr {thr} {NAMES[tA]}-{NAMES[tB]}"
    ob.set_libm_trig(True)
    try:
        op, oc = ob.collide_batch(st, sp, pos, orn, threshold=thr)
        ok = ob.last_batch_flags(len(st)) == 0
        rp, rc = ob.ref_collide_batch(st[ok], sp[ok], pos[ok], orn[ok], threshold=thr)
    finally:
        ob.set_libm_trig(False)
    flagged = 1.0 - ok.mean()
    if flagged:
        print(f"[edges] {what}: flagged {flagged:.2%}")
    assert (tA == P and tB == P) or ok.all(), what
    assert flagged <= (MAX_FLAGGED_LATTICE if cls == "lattice" else MAX_FLAGGED), (what, flagged)
    _assert_caps(op, oc, what)
    assert np.array_equal(oc[ok], rc), (what, "counts", np.flatnonzero(oc[ok] != rc)[:8])
    used = _used(rc)
    assert np.array_equal(op[ok][used].view(np.uint32), rp[used].view(np.uint32)), what   # NaN included: both sides are x86


@needs_engine
@pytest.mark.parametrize("tA,tB", COMBOS, ids=lambda t: NAMES[t])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_oracle_collide_matches_the_engine_on_degenerate_pairs(case, tA, tB):
    """The batches of the device leg through the oracle and through the real edyn::collide overloads: counts and every used bit."""
    _assert_oracle_matches_engine(case[0], case[1], tA, tB)


@needs_engine
@pytest.mark.parametrize("other", POLY_PARTNERS, ids=lambda t: NAMES[t])
@pytest.mark.parametrize("case", CASES_POLY, ids=_case_id)
def test_oracle_polyhedron_collide_matches_the_engine_on_degenerate_pairs(case, other):
    """As above for the polyhedron routines in both argument orders. Pairs of polyhedra without an edge pair that spans a Minkowski
    face are left out, as in test_polyhedron_collide_matches_the_reference_routines: the reference reads uninitialised variables there.
    Such pairs are under 2 % of a batch except on the grid: with identity orientations the edges of two prisms or boxes are parallel
    as a rule, not by accident, so there the share is capped at 40 % - the rest still is thousands of compared pairs."""
    for tA, tB in _orders(other):
        _assert_oracle_matches_engine(case[0], case[1], tA, tB)
