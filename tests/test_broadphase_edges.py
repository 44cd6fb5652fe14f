"""The broadphase on DEGENERATE layouts and at its thresholds: the device's pair set and body order (broadphase.hip) against the
oracle's, the oracle's against the real engine's, and the oracle's against a plain-numpy statement of the definition.

Everything downstream is compared with the oracle bit for bit and rests on the pair set S_t and each manifold's body order being exact.
The ordinary scenes (piles, pyramids, heaps, chains near the origin) never show the broadphase what tests/bplayouts.py builds:
  * pairs whose gap IS the creation / separation threshold to within two units in the last place, their faces on either side of a power
    of two, where `the higher index's grown box reaches the other` and `the lower index's grown box reaches the other`
    round differently - the only input on which a manifold's body[0] is the lower index, and on which the keep test depends on the order;
  * Morton input without extent (coincident centres, a line, a sheet, clusters of equal codes, one outlier that squeezes everyone
    else into one cell), where the Karras tree is a tree over index bits and the walks' stacks and lists fill;
  * owners with exactly 63 / 64 / 65 partners and 127 / 128 / 129 candidates (kOwnCap, kListCap);
  * every kernel granularity in the number of procedural and static bodies;
  * coordinates of 1e3 .. 1e6, where the list margins are below one unit in the last place;
  * scenes in motion whose candidate lists expire every few steps (a gas), or in every step (bullets).

Three legs, as in test_collide_edges.py:
  * oracle against bplayouts.definition (CPU, no engine needed): guards the checker's own dynamic tree before the device is held to it;
  * oracle against the real engine (CPU; skipped where oracle/_ref was not built);
  * device against oracle (gpu): the broadphase stage alone on every layout, whole steps on those that need motion.
What a layout must contain to be worth running is asserted on the oracle's output or the scene's arrays alone, never on the device's.
"""
import functools

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from edyn_amd._capi import STAGE_BROADPHASE
from oracle import binding as ob
import bplayouts as bl

VARIANTS = ("dynamic", "static", "kinematic")
GAPS = {"create": bl.D_CREATE, "keep": bl.D_KEEP}


# ------------------------------------------------------------------------------------------------ the cases
# group -> [(case name, builder)]; a builder returns a scene, or (scene, pos2) for the two-phase `keep` cases
def _groups():
    g = {}
    for v in VARIANTS:
        g[f"straddle-{v}"] = [(f"straddle-{v}-{gn}-P{P}", functools.partial(lambda P, d, v: bl.straddle(P, d, v)[0], P, GAPS[gn], v))
                              for P, gn in bl.STRADDLE_CASES]
        g[f"keep-{v}"] = [(f"keep-{v}-P{P}", functools.partial(bl.keep, P, v)) for P in bl.KEEP_P]
    g["coincident"] = [(f"coincident-{n}", functools.partial(bl.coincident, n)) for n in (2, 65, 66, 130, 200)]
    g["line-sheet"] = [("line", bl.line), ("sheet", bl.sheet)]
    g["clusters"] = [("clusters", bl.clusters)]
    g["outlier"] = [("outlier-first", functools.partial(bl.outlier, True)), ("outlier-last", functools.partial(bl.outlier, False))]
    for where in ("first", "last", "static", "kinematic"):
        g[f"giant-{where}"] = [(f"giant-{where}", functools.partial(bl.giant, where))]
    g["owner_k"] = [(f"owner-{k}", functools.partial(bl.owner_k, k)) for k in (63, 64, 65)]
    g["list_k"] = [(f"list-{k}", functools.partial(bl.owner_k, k)) for k in (127, 128, 129)]
    for ns in bl.STATICS:
        g[f"counts-statics{ns}"] = [(f"counts-{n}-statics{ns}", functools.partial(bl.counts, n, ns)) for n in bl.COUNTS]
    g["counts-statics-only"] = [("counts-0-statics4", functools.partial(bl.counts, 0, 4))]
    g["far"] = [(f"far-{w}-T{T}", functools.partial(bl.far, float(T), w)) for T in (1e3, 1e4, 131072, 1048576) for w in ("pile", "chain")]
    return g


GROUPS = _groups()
# whole-step layouts, for the one-step engine leg and the definition leg (their first broadphase)
MOVING = [(f"gas-{c}", functools.partial(bl.gas, ctr)) for c, ctr in bl.GAS_CENTRES.items()] + [("bullets", bl.bullets)]
CPU_GROUPS = dict(GROUPS, moving=MOVING)
MAX_MANIFOLDS = 1 << 16   # coincident-200 has 19 900 pairs; the default capacity is 16 per body


def oracle_world(scene, sleeping=False):
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(scene)
    if sleeping:
        o.set_sleeping(True)
    return o


def gpu_world(scene, **kw):
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, max_manifolds=MAX_MANIFOLDS, **kw))
    w.set_scene(scene)
    return w


def _built(build):
    r = build()
    return r if isinstance(r, tuple) else (r, None)


def _move(world, pos2):
    _, orn, lv, av = world.get_state()
    world.set_state(pos2, orn, lv, av)


def _oracle_stage(scene, pos2):
    """The oracle's broadphase from an empty manifold set, then (keep) once more after the move. Returns
    [(aabb, bodies in canonical order, pair keys)] per phase."""
    o = oracle_world(scene)
    out = []
    for phase in range(2 if pos2 is not None else 1):
        if phase:
            _move(o, pos2)
            o.refresh_derived()
        o.run_stage(0)
        m = o.get_manifolds()
        out.append((o.get_derived()[0].copy(), m["body"].copy(), o.get_pairs()))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_group(group):
    """What the oracle's broadphase makes of every case of a group: computed once, shared by the legs, never changed."""
    return [(name,) + _built(build) + (_oracle_stage(*_built(build)),) for name, build in CPU_GROUPS[group]]


# ------------------------------------------------------------------------------------------------ oracle against the definition
@pytest.mark.parametrize("group", list(CPU_GROUPS))
def test_oracle_broadphase_matches_the_definition(group):
    """One broadphase from an empty manifold set (and the keep move): pair keys and body order of the oracle, whose broadphase walks
    the reference's dynamic tree (fattened leaves, also at 1e6), equal the definition's, which uses no tree."""
    for name, scene, pos2, phases in _oracle_group(group):
        prev = None
        for k, (aabb, body, _) in enumerate(phases):
            want = bl.definition(aabb, scene["kind"], prev)
            got = bl.canon_bodies({"body": body})
            assert np.array_equal(got, want), (name, k, len(got), len(want))
            prev = got


# ------------------------------------------------------------------------------------------------ what the layouts must contain
def _lower_first(body):
    return int((body[:, 0] < body[:, 1]).sum()) if len(body) else 0


def test_straddle_pairs_reach_the_lower_index_first_branch():
    """On the oracle's output: at every P of the table at least 10 manifolds whose body[0] is the LOWER index (the branch of
    consider_pair that only rounding reaches), and over all P between 40 % and 75 % of the pairs created at the creation gap. (A P
    that yields none is decoration and leaves bplayouts.STRADDLE_P; 0, 0.5 and 1024 did.) The static and kinematic variants are printed."""
    created = total = 0
    for v in VARIANTS:
        for name, scene, _, phases in _oracle_group(f"straddle-{v}"):
            body, npairs = phases[0][1], len(scene["kind"]) // 2
            n = _lower_first(body)
            print(f"[bp edges] {name}: {len(body)} of {npairs} created, body[0] is the lower index in {n}")
            if v == "dynamic":
                assert n >= 10, (name, n)
                if "-create-" in name:
                    created += len(body); total += npairs
    print(f"[bp edges] straddle, both dynamic, creation gap, all P: created share {created / total:.1%}")
    assert 0.40 <= created / total <= 0.75, created / total


def test_keep_pairs_depend_on_the_body_order():
    """On the oracle's AABBs after the move: at least 10 pairs over the class that are kept in one body order and dropped in the other;
    and at least 10 of them in manifolds whose body[0] is the LOWER index - there the box that the keep test grows is not the owner's,
    which is the only input that tells `body[0]'s box` from `the querying body's box`. (The first phase sits at the creation gap for
    that reason: at a gap of 0.01 every pair is created by the higher index.) Measured: 18 such manifolds, all at P = -0.25."""
    dependent = swapped_dependent = 0
    for v in VARIANTS:
        for name, scene, _, phases in _oracle_group(f"keep-{v}"):
            body1, aabb2, body2 = phases[0][1], phases[1][0], phases[1][1]
            assert len(body1) > 0.4 * (len(scene["kind"]) // 2), (name, len(body1))
            mn, mx = aabb2[:, :3], aabb2[:, 3:]
            a, b = body1[:, 0], body1[:, 1]

            def holds(x, y):
                return np.all(((mn[x] - bl.D_KEEP) <= mx[y]) & (mn[y] <= (mx[x] + bl.D_KEEP)), axis=1)
            dep = holds(a, b) != holds(b, a)
            low_first = (a < b) & (scene["kind"][a] == scenes.KIND_DYNAMIC) & (scene["kind"][b] == scenes.KIND_DYNAMIC)
            dependent += int(dep.sum()); swapped_dependent += int((dep & low_first).sum())
            print(f"[bp edges] {name}: {len(body1)} created, {len(body2)} kept, {int(dep.sum())} depend on the body order, "
                  f"{int((dep & low_first).sum())} of those with the lower index first")
    print(f"[bp edges] keep: {dependent} order-dependent pairs over the class, {swapped_dependent} with the lower index first")
    assert dependent >= 10 and swapped_dependent >= 10, (dependent, swapped_dependent)


def _assert_owner_counts(scene, aabb, k, what):
    owner = len(scene["kind"]) - 1
    partners = bl.partner_count(aabb, owner)
    cands = [bl.candidate_count(aabb, scene["linvel"], scene["angvel"], owner, la) for la in bl.LOOKAHEAD_RANGE]
    print(f"[bp edges] {what}: owner {owner} has {partners} partners, {cands} candidates at a look-ahead of {bl.LOOKAHEAD_RANGE}")
    assert partners == k and cands == [k, k], (what, partners, cands)


def test_owner_and_list_counts_are_exact():
    """Partner and candidate counts of the owner, in numpy from the oracle's AABBs (the candidates by k_bp_refit's slack formula, at
    both ends of the look-ahead's range): exactly k."""
    for group in ("owner_k", "list_k"):
        for name, scene, _, phases in _oracle_group(group):
            _assert_owner_counts(scene, phases[0][0], int(name.split("-")[1]), name)


# ------------------------------------------------------------------------------------------------ oracle against the real engine
needs_engine = pytest.mark.skipif(ob.ref() is None, reason="oracle/_ref/libedynref.so not built (needs the reference's source at build time)")


@needs_engine
@pytest.mark.parametrize("group", list(CPU_GROUPS))
def test_oracle_broadphase_matches_the_engine(group):
    """One whole step of the real engine and of the oracle on every layout: the same pairs in the same body order. The keep cases then
    move (set_state leaves the AABBs to the end of the next step, on both sides) and step twice; the pairs do not move on their own
    (asserted), so the second step's broadphase sees exactly the boxes the generator aimed at."""
    for name, build in CPU_GROUPS[group]:
        scene, pos2 = _built(build)
        ref = ob.RefWorld(vel_iters=10)
        ref.add_bodies(scene)
        o = oracle_world(scene)
        ref.step(1); o.step(1)
        rb, obd = bl.canon_bodies(ref.get_manifolds()), bl.canon_bodies(o.get_manifolds())
        assert np.array_equal(rb, obd), (name, len(rb), len(obd))
        if pos2 is not None:
            for w in (ref, o):
                assert np.array_equal(w.get_state()[0], scene["pos"]), (name, "a pair at the creation gap moved")
                _move(w, pos2)
                w.step(2)
                assert np.array_equal(w.get_state()[0], pos2), (name, "a pair at the separation gap moved")
            rb, obd = bl.canon_bodies(ref.get_manifolds()), bl.canon_bodies(o.get_manifolds())
            assert np.array_equal(rb, obd), (name, "after the move", len(rb), len(obd))
            assert 0 < len(obd) < len(scene["kind"]) // 2, name


# ------------------------------------------------------------------------------------------------ device against oracle: the stage
def _assert_stage(g, phase, what):
    _, body, pairs = phase
    assert np.array_equal(g.get_pairs(), pairs), (what, "pair keys")
    assert np.array_equal(g.get_manifolds()["body"], body), (what, "body order")


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_device_broadphase_stage_matches_the_oracle(group):
    """The broadphase stage alone from an empty manifold set (and again after the keep move, over the first phase's manifolds): pair
    keys and the manifolds' body columns equal the oracle's."""
    for name, scene, pos2, phases in _oracle_group(group):
        g = gpu_world(scene)
        g.run_stages(STAGE_BROADPHASE)
        _assert_stage(g, phases[0], name)
        if pos2 is not None:
            _move(g, pos2)
            g.refresh_derived()
            g.run_stages(STAGE_BROADPHASE)
            _assert_stage(g, phases[1], name + " after the move")


STAGE_PATHS = [("coincident-65", functools.partial(bl.coincident, 65), False), ("coincident-66", functools.partial(bl.coincident, 66), True),
               ("coincident-200", functools.partial(bl.coincident, 200), True),
               ("giant-last", functools.partial(bl.giant, "last"), True), ("owner-65", functools.partial(bl.owner_k, 65), True),
               ("owner-63", functools.partial(bl.owner_k, 63), False), ("owner-64", functools.partial(bl.owner_k, 64), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,build,surplus", STAGE_PATHS, ids=[c[0] for c in STAGE_PATHS])
def test_surplus_path_runs_exactly_beyond_the_owner_capacity(name, build, surplus):
    """PAIR_SURPLUS (the unsorted surplus and its sort) shows for an owner of 65 and more partners, and not for one of 63 or 64. Among n
    coincident bodies the last one owns n - 1 pairs: 65 of them fill its 64 keys exactly, 66 are the first to spill."""
    g = gpu_world(build())
    g.run_stages(STAGE_BROADPHASE)
    assert ("PAIR_SURPLUS" in g.debug_paths()) == surplus, (name, sorted(g.debug_paths()))


# ------------------------------------------------------------------------------------------------ device against oracle: whole steps
def _lockstep(name, scene, steps, need=(), clear=(), sleeping=False, at_ends=None, churn=None):
    """Device and oracle step together: pair keys, the state's bit patterns and the manifolds' body columns after every step, whole
    manifolds at the end; then the paths the device must (not) have taken. at_ends(o): a check on the oracle at the first and last
    step; churn: minimum number of manifolds created and destroyed over the run, counted on the oracle's pair keys."""
    from test_gpu_parity import assert_manifolds_equal
    g, o = gpu_world(scene, sleeping=sleeping), oracle_world(scene, sleeping=sleeping)
    created = destroyed = 0
    before = set()
    for s in range(steps):
        g.step_simulation(1); o.step(1)
        op = o.get_pairs()
        assert np.array_equal(g.get_pairs(), op), (name, s, "pair keys")
        for a, b, f in zip(g.get_state(), o.get_state(), ("pos", "orn", "linvel", "angvel")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, s, f)
        assert np.array_equal(g.get_manifolds()["body"], o.get_manifolds()["body"]), (name, s, "body order")
        now = set(op.tolist())
        created += len(now - before); destroyed += len(before - now)
        before = now
        if at_ends is not None and s in (0, steps - 1):
            at_ends(o, f"{name} step {s}")
    assert_manifolds_equal(g.get_manifolds(), o.get_manifolds(), what=name)
    paths = g.debug_paths()
    print(f"[bp edges] {name}: {steps} steps, {created} manifolds created, {destroyed} destroyed, {len(before)} at the end; paths {sorted(paths)}")
    if churn is not None:
        assert created >= churn and destroyed >= churn, (name, created, destroyed)
    assert set(need) <= paths and not (set(clear) & paths), (name, sorted(paths))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("pile", "chain"))
@pytest.mark.parametrize("T", (1e3, 1e4), ids=("T1e3", "T1e4"))
def test_steps_far_from_the_origin_match_the_oracle(T, which):
    """30 steps under gravity of the mixed pile and of the chain of 257 at (T, -3T, 2T). At 1e4 the lists must have been both reused
    and rebuilt on the device's own flag."""
    _lockstep(f"far-{which}-T{T:g}", bl.far(T, which), 30, need=("LISTS_KEPT", "LISTS_MOVED") if T == 1e4 else ())


@pytest.mark.gpu
@pytest.mark.parametrize("centre", list(bl.GAS_CENTRES))
def test_gas_steps_match_the_oracle(centre):
    """40 steps of 1 500 spheres in flight: at least 200 manifolds created and 200 destroyed, lists reused and rebuilt."""
    _lockstep(f"gas-{centre}", bl.gas(bl.GAS_CENTRES[centre]), 40, need=("LISTS_KEPT", "LISTS_MOVED"), churn=200)


@pytest.mark.gpu
def test_bullet_steps_match_the_oracle():
    """12 steps of the grid with eight bodies crossing it at 5 m a step: the lists expire on the device's flag, the look-ahead adapts."""
    _lockstep("bullets", bl.bullets(), 12, need=("LISTS_MOVED", "LOOKAHEAD_CHANGED"))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (65, 66))
def test_coincident_steps_match_the_oracle(n):
    """5 steps of n coincident bodies, which the contacts push apart: every owner's key list and every candidate list at or over its
    capacity in the first step (2 080 / 2 145 pairs), 1 525 pairs in the second, fewer each step. With 66 the surplus path runs.

    Found by n = 65: the serial colour bucket (the contacts beyond the 62 conflict-free colours) then holds 33 four-point and 63
    one-point manifolds that share bodies. The device walked the bucket in its sorted order - point-count groups first - where the
    checker, and DESIGN, take it in canonical order: all 65 positions differed after the first step (first body: x 0.51347584 against
    0.50149804). With 41 .. 64 and 66 bodies the few four-point manifolds of the bucket happened not to matter. Fixed in the two serial
    kernels (solver.hip, serial_next)."""
    _lockstep(f"coincident-{n}", bl.coincident(n), 5, need=("PAIR_SURPLUS",) if n >= 66 else (), clear=() if n >= 66 else ("PAIR_SURPLUS",))


def _serial_bucket_mix(o):
    """(manifolds in the serial bucket, point counts in it, bodies shared between manifolds of different point counts) of an oracle."""
    m = o.get_manifolds()
    ser = m[(m["colour"] == 62) & (m["num_points"] > 0)]
    counts = sorted(set(ser["num_points"].tolist()))
    by = {c: set(ser["body"][ser["num_points"] == c].ravel().tolist()) for c in counts}
    shared = set().union(*[by[a] & by[b] for a in counts for b in counts if a < b]) if len(counts) > 1 else set()
    return len(ser), counts, len(shared)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (65, 97))
def test_serial_bucket_of_mixed_point_counts_matches_the_oracle(n):
    """n coincident boxes and spheres with drawn velocities of up to 1 m/s, 4 steps: the serial bucket holds manifolds of one and of
    four points that share bodies (asserted on the oracle after the first step) and their contacts carry impulses (asserted too), so
    both serial kernels - velocity and position - have an order to get wrong."""
    scene = bl.coincident(n, speed=1.0)

    def mixed(o, what):
        size, counts, shared = _serial_bucket_mix(o)
        print(f"[bp edges] {what}: serial bucket of {size} manifolds, point counts {counts}, {shared} bodies shared between counts")
        if what.endswith("step 0"):
            assert size >= 64 and len(counts) >= 2 and shared >= 10, (what, size, counts, shared)
            m = o.get_manifolds()
            ser = m[(m["colour"] == 62) & (m["num_points"] > 0)]
            assert (ser["pt"]["normal_impulse"] > 0).any(axis=1).sum() >= 10, what   # (measured: 11 at n = 65, 123 at n = 97)
    _lockstep(f"coincident-{n}-moving", scene, 4, at_ends=mixed)


@pytest.mark.gpu
@pytest.mark.parametrize("k,sleeping", [(63, False), (64, False), (65, False), (127, False), (128, False), (129, False),
                                        (127, True), (128, True), (129, True)])
def test_steps_at_the_owner_and_list_capacities_match_the_oracle(k, sleeping):
    """10 steps with the small spheres adrift at 0.05 m/s: the lists are reused, and the owner's counts are k at the first and the last
    step (from the oracle's boxes and velocities). With island sleeping the lists also carry the higher-index candidates."""
    scene = bl.owner_k(k, speed=0.05)

    def counts_hold(o, what):
        _, _, lv, av = o.get_state()
        _assert_owner_counts(dict(scene, linvel=lv, angvel=av), o.get_derived()[0], k, what)
    _lockstep(f"owner-{k}{'-sleeping' if sleeping else ''}", scene, 10, need=("LISTS_KEPT",) + (("PAIR_SURPLUS",) if k >= 65 else ()),
              clear=() if k >= 65 else ("PAIR_SURPLUS",), sleeping=sleeping, at_ends=counts_hold)
