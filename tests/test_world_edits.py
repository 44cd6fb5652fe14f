"""Edits of a running multi-device world (edynhip_world_add_bodies / _remove_bodies / _add_joints / _remove_joints / _edit_joint /
_edit_exclusion / _set_state / _set_params; MultiWorld.add_scene ...): 1, 2 and 3 shards on device 0 against ONE context that holds the
whole scene and receives the same edits through World.add_scene, remove_bodies, add_joints ...

The contract: after any sequence of edits and steps the world returns bit for bit what the one context returns - state of the live
bodies, every field of the manifolds, the sleeping tags - after EVERY step. Which path an edit took (in place, a shard rebuilt with
head-room, a re-partition because islands of two shards came together) is read from MultiWorld.get_edit_stats()."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd.multi import MultiWorld

pytestmark = pytest.mark.gpu
SHARDS = [1, 2, 3]
ERR_INVALID = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PILE_TOP = 0.505 + 3 * 1.005 + 0.5     # scenes._lattice: four layers of unit boxes


def _cfg(**kw):
    return edyn_amd.init_config(num_solver_velocity_iterations=10, **kw)


def _bodies(rows):
    """A scene dict of new bodies: rows of dict(kind=, pos=, shape=, param=, linvel=)."""
    s = scenes._empty(len(rows))
    for i, r in enumerate(rows):
        s["kind"][i] = r.get("kind", scenes.KIND_DYNAMIC)
        s["pos"][i] = r["pos"]
        s["linvel"][i] = r.get("linvel", (0, 0, 0))
        s["shape_type"][i] = r["shape"]
        s["shape_param"][i, :len(r["param"])] = r["param"]
    return s


def _site(sx, sz, nx, nz, pitch=8.0):
    return np.array([(sx - (nx - 1) / 2.0) * pitch, 0.0, (sz - (nz - 1) / 2.0) * pitch], np.float32)


def _spawn3():
    """A box 1 m above the pile of site 0, a sphere 30 m from everything, a static box 2 cm beside the pile of site 1 (mini_piles(3, 2))."""
    s0, s1 = _site(0, 0, 3, 2), _site(1, 0, 3, 2)
    return _bodies([dict(pos=(s0[0], PILE_TOP + 1.0 + 0.5, s0[2]), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5)),
                    dict(pos=(0.0, 1.0, 40.0), shape=scenes.SHAPE_SPHERE, param=(0.5,)),
                    dict(kind=scenes.KIND_STATIC, pos=(s1[0] + 2.05 + 0.5, 0.5, s1[2]), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5))])


class Pair:
    """The world under test and the one context it has to equal; every step is compared."""

    def __init__(self, scene, shards, room_bodies=64, room_joints=64, **kw):
        n, nj = len(scene["kind"]), len(scene.get("joints") or [])
        self.w = edyn_amd.World(_cfg(max_bodies=n + room_bodies, max_joints=nj + room_joints, **kw))
        self.w.set_scene(scene); scenes.apply_figure_settings(self.w, scene)
        self.mw = MultiWorld(_cfg(**kw), devices=[0] * shards)
        self.mw.set_scene(scene)
        self.sleeping = bool(kw.get("sleeping"))
        self.dead = []
        self.steps = 0

    def compare(self, what=None):
        what = (what, self.steps)
        assert self.mw.n == self.w.n, what
        live = np.ones(self.w.n, bool); live[self.dead] = False
        for a, b in zip(self.mw.get_state(), self.w.get_state()):
            assert np.array_equal(a[live], b[live]), what
        gm, sm = self.mw.get_manifolds(), self.w.get_manifolds()
        assert len(gm) == len(sm), what
        for f in ("body", "num_points", "colour"):
            assert np.array_equal(gm[f], sm[f]), (what, f)
        for f in _capi.POINT_DTYPE.names:
            assert np.array_equal(gm["pt"][f], sm["pt"][f]), (what, f)
        if self.sleeping:
            assert np.array_equal(self.mw.get_asleep()[live], np.asarray(self.w.get_asleep(), np.uint8)[live]), what

    def step(self, k=1, what=None):
        for _ in range(k):
            self.w.step_simulation(1); self.mw.step_simulation(1)
            self.steps += 1
            self.compare(what)

    def add(self, scene):
        fs = self.w.add_scene(scene)
        fb, fj = self.mw.add_scene(scene)
        assert fb == fs
        return fb

    def remove(self, idx):
        self.w.remove_bodies(idx); self.mw.remove_bodies(idx)
        self.dead = sorted(set(self.dead) | set(int(i) for i in idx))

    def add_joints(self, joints):
        a, b = self.w.add_joints(joints), self.mw.add_joints(joints)
        assert a == b
        return a


def _lightest(part, kind, shards):
    load = np.bincount(part[(part >= 0) & (kind == scenes.KIND_DYNAMIC)], minlength=shards)
    return int(np.argmin(load)), load


# ---- 1. spawn ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_spawn_in_place(shards):
    scene = scenes.mini_piles(3, 2)
    p = Pair(scene, shards)
    p.step(40)
    n = p.mw.n
    part = p.mw.get_partition()
    r_box, load = _lightest(part, scene["kind"], shards)
    load[r_box] += 1
    r_sphere = int(np.argmin(load))
    before = p.mw.get_edit_stats()
    assert p.add(_spawn3()) == n and p.mw.n == n + 3
    st = p.mw.get_edit_stats()
    assert st["edits"] == before["edits"] + 1 and st["in_place"] == before["in_place"] + 1, st
    assert st["shard_rebuilds"] == 0 and st["repartitions_by_edit"] == 0, st
    assert st["approach_checks_by_edit"] == (1 if shards > 1 else 0), st
    part = p.mw.get_partition()
    assert part[n + 2] == -1 and part[n] == r_box and part[n + 1] == r_sphere, (part[n:], r_box, r_sphere)
    p.compare("after the add")
    p.step(60)
    st = p.mw.get_edit_stats()
    assert st["shard_rebuilds"] == 0 and st["repartitions_by_edit"] == 0, st
    assert p.mw.get_state()[0][n, 1] < PILE_TOP + 0.6, "the box has landed on the pile"


# ---- 2. a spawn that bridges two shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
def test_spawn_bridges_two_shards(shards):
    scene = scenes.mini_piles(3, 2)
    p = Pair(scene, shards)
    p.step(20)
    part = p.mw.get_partition()
    owner = {(sx, sz): int(part[1 + 64 * (sz * 3 + sx)]) for sx in range(3) for sz in range(2)}
    pick = None
    for (sx, sz), r in sorted(owner.items()):
        for other in ((sx + 1, sz), (sx, sz + 1)):
            if pick is None and other in owner and owner[other] != r:
                pick = ((sx, sz), other)
    if pick is None:
        pytest.skip("every pair of neighbouring sites shares a shard")
    a, b = pick
    ca, cb = _site(a[0], a[1], 3, 2), _site(b[0], b[1], 3, 2)
    mid = (ca + cb) / 2
    half = (5.0, 0.1, 0.3) if a[1] == b[1] else (0.3, 0.1, 5.0)       # a beam lying across the two piles, 1 cm above them
    n = p.mw.n
    before = p.mw.get_stats()["repartitions"]
    p.add(_bodies([dict(pos=(mid[0], PILE_TOP + 0.11, mid[2]), shape=scenes.SHAPE_BOX, param=half)]))
    st = p.mw.get_edit_stats()
    assert st["repartitions_by_edit"] >= 1 and p.mw.get_stats()["repartitions"] > before, st     # before any step
    part = p.mw.get_partition()
    fa, fb = 1 + 64 * (a[1] * 3 + a[0]), 1 + 64 * (b[1] * 3 + b[0])
    assert part[fa] == part[fb] == part[n], (part[fa], part[fb], part[n])
    p.compare("after the add")
    p.step(60)
    part = p.mw.get_partition()
    assert len(set(part[fa:fa + 64]) | set(part[fb:fb + 64]) | {part[n]}) == 1


# ---- 3. remove -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_remove_wakes_one_pile(shards):
    scene = scenes.mini_piles(3, 2)
    p = Pair(scene, shards, sleeping=True)
    p.step(10)
    n = p.mw.n
    static_box = p.add(_spawn3()) + 2
    dyn = scene["kind"] == scenes.KIND_DYNAMIC
    # (measured on this scene: the six piles fall asleep between steps 313 and 387 - island_time_to_sleep is 2 s = 120 steps after the
    # last body of a pile has come to rest - so the cap is 420 steps, not 200; every one of them is compared)
    while p.steps < 420 and not p.mw.get_asleep()[:n][dyn].all():
        p.step(1)
    asleep = p.mw.get_asleep()
    assert asleep[:n][dyn].all(), "the piles went to sleep"
    site2 = np.arange(1 + 64 * 2, 1 + 64 * 3)
    bottom = int(site2[np.argmin(p.mw.get_state()[0][site2, 1])])
    before = p.mw.get_edit_stats()
    p.remove([bottom, static_box])
    st = p.mw.get_edit_stats()
    assert st["in_place"] == before["in_place"] + 1 and st["shard_rebuilds"] == 0 and st["repartitions_by_edit"] == 0, st
    part = p.mw.get_partition()
    assert part[bottom] == -1 and part[static_box] == -1
    others = np.concatenate([np.arange(1 + 64 * s, 1 + 64 * (s + 1)) for s in (0, 3, 4, 5)])
    rest = site2[site2 != bottom]
    p.step(1)
    for asleep in (p.mw.get_asleep(), np.asarray(p.w.get_asleep(), np.uint8)):
        assert (asleep[rest] == 0).sum() >= 32, "the island that lost a box is awake"   # (a settled site is more than one island; brick-laid, it moves by less than a millimetre)
        assert asleep[others].all(), "the piles nobody touched stay asleep"
    p.step(39)
    assert p.mw.get_asleep()[others].all() and np.asarray(p.w.get_asleep(), np.uint8)[others].all()
    first = p.add(_bodies([dict(pos=(0.0, 1.0, -40.0), shape=scenes.SHAPE_SPHERE, param=(0.5,))]))
    assert first == n + 3, "a removed body's index is not reused"
    p.remove([bottom])                                  # again: accepted, nothing happens, as on one context
    p.step(10)


# ---- 4. joints -----------------------------------------------------------------------------------------------------------------------
def _to_local(q, v):
    """v rotated by the inverse of quaternion q (xyzw)."""
    qc = np.array([-q[0], -q[1], -q[2], q[3]], np.float32)
    return tuple(float(x) for x in scenes._quat_rotate(qc, np.asarray(v, np.float32)))


def _joint_between(state, jt, a, b):
    """A joint whose pivots coincide now: the origin of body a, seen from both bodies."""
    pos, orn = state[0], state[1]
    return (jt, int(a), int(b), (0.0, 0.0, 0.0), _to_local(orn[b], pos[a] - pos[b]), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0))


@pytest.mark.parametrize("shards", SHARDS)
def test_joints_across_and_inside_shards(shards):
    links = 4
    scene = scenes.c5_chains(num_chains=4, links=links)
    p = Pair(scene, shards)
    p.step(20)
    part = p.mw.get_partition()
    last = [c * (links + 1) + links for c in range(4)]
    pick = next(((x, y) for x in last for y in last if x < y and part[x] != part[y]), None)
    if shards > 1:
        assert pick is not None, "four equal chains on two or three shards: some two are apart"
    a, b = pick or (last[0], last[1])
    state = p.mw.get_state()
    before = p.mw.get_edit_stats()
    first = p.add_joints([_joint_between(state, scenes.JOINT_HINGE, a, b)])
    assert first == len(scene["joints"])
    st = p.mw.get_edit_stats()
    if shards > 1:
        assert st["repartitions_by_edit"] >= before["repartitions_by_edit"] + 1, st
        part = p.mw.get_partition()
        assert part[a] == part[b]
    p.compare("after the hinge")
    p.step(10)
    # a point joint inside one chain: in place
    state = p.mw.get_state()
    before = p.mw.get_edit_stats()
    p.add_joints([_joint_between(state, scenes.JOINT_POINT, 1, 3)])
    st = p.mw.get_edit_stats()
    assert st["in_place"] == before["in_place"] + 1 and st["repartitions_by_edit"] == before["repartitions_by_edit"] and st["shard_rebuilds"] == 0, st
    p.step(40)
    # remove a mid-chain joint: in place; the applied impulses and angles of every other joint survive (bit-equal steps)
    before = p.mw.get_edit_stats()
    gone = 1 * links + 2
    p.w.remove_joints([gone]); p.mw.remove_joints([gone])
    st = p.mw.get_edit_stats()
    assert st["in_place"] == before["in_place"] + 1 and st["repartitions_by_edit"] == before["repartitions_by_edit"] and st["shard_rebuilds"] == 0, st
    p.step(20)
    # new limits on an old hinge
    hinge = 2 * links + 1
    assert scene["joints"][hinge][0] == scenes.JOINT_HINGE
    limits = (-0.4, 0.4, 0.0, 0.05, 30.0, 0, 0, 0, 0, 0)
    p.w.set_joint_params(hinge, limits); p.mw.set_joint_params(hinge, limits)
    p.step(30)
    assert p.mw.get_edit_stats()["shard_rebuilds"] == 0


# ---- 5. a rag doll dropped onto a running pile ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_ragdoll_dropped_onto_a_pile(shards):
    scene = scenes.mini_piles(2, 1)
    fig = scenes.figures(scenes.load_figure(os.path.join(GOLDEN, "ragdoll_capsule.npz")), 1, 1, floor=False, hip_height=PILE_TOP + 1.5 + 1.25)
    fig["pos"][:, 0] += _site(0, 0, 2, 1)[0]
    nfb, nfj = len(fig["kind"]), len(fig["joints"])
    p = Pair(scene, shards, room_bodies=nfb + 8, room_joints=nfj + 8)
    p.step(30)
    # the one context: bodies, then the joints with the hinges' parameters, the cone / cvjoint definitions, the exclusions
    fb = p.w.add_scene(fig)
    params = dict(fig["hinge_params"])
    fj = p.w.add_joints([(j[0], j[1] + fb, j[2] + fb) + tuple(j[3:]) + ((tuple(params[k]),) if k in params else ()) for k, j in enumerate(fig["joints"])])
    for j, fa, fbm, q in fig["joint_defs"]:
        p.w.set_joint_definition(fj + j, fa, fbm, q)
    for x, y in fig["exclusions"]:
        p.w.exclude_collision(fb + int(x), fb + int(y))
    assert p.mw.add_scene(fig) == (fb, fj) and p.mw.n == p.w.n and p.mw.nj == p.w.nj
    part = p.mw.get_partition()
    assert len(set(part[fb:fb + nfb])) == 1, "a figure is one island: its bodies share a shard"
    p.compare("after the add")
    p.step(60)
    assert p.mw.get_state()[0][fb:fb + nfb, 1].min() < PILE_TOP + 1.0, "the figure has fallen onto the pile"


# ---- 6. capacity fallback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_add_beyond_capacity_rebuilds_the_shard(shards):
    scene = scenes.mini_piles(2, 1)
    p = Pair(scene, shards, room_bodies=420)
    p.step(30)
    n = p.mw.n
    grid = [dict(pos=(-19.0 + 2.0 * (k % 20), 0.3, 30.0 + 2.0 * (k // 20)), shape=scenes.SHAPE_SPHERE, param=(0.25,)) for k in range(400)]
    assert p.add(_bodies(grid)) == n
    st = p.mw.get_edit_stats()
    assert st["shard_rebuilds"] >= 1 and st["in_place"] == 0, st
    assert sum(p.mw.get_stats()["bodies_per_shard"]) == n + 400
    p.compare("after the add")
    p.step(30)      # the settled piles included: their warm start went through the carry


# ---- 7. contact events across edits --------------------------------------------------------------------------------------------------
def _idless(ev):
    a = np.stack([ev["step"].astype(np.int64), ev["type"].astype(np.int64), ev["body"][:, 0].astype(np.int64), ev["body"][:, 1].astype(np.int64)], 1) \
        if len(ev) else np.zeros((0, 4), np.int64)
    return a[np.lexsort(a.T[::-1])]


def _with_ids(ev, kind, rename=None):
    e = ev[ev["type"] == kind]
    ids = [int(x) for x in e["point_id"]]
    if rename is not None:
        missing = [hex(x) for x in ids if x not in rename]
        assert not missing, ("event ids the id tables never showed", missing[:5])
        ids = [rename[x] for x in ids]
    return sorted(zip(e["step"].tolist(), e["body"][:, 0].tolist(), e["body"][:, 1].tolist(), ids))


@pytest.mark.parametrize("shards", SHARDS)
def test_contact_events_across_edits(shards):
    scene = scenes.mini_piles(3, 2)
    p = Pair(scene, shards, contact_events=True)
    rename, back = {0: 0}, {0: 0}
    created, destroyed = _capi.EVENT_POINT_CREATED, _capi.EVENT_POINT_DESTROYED

    def tables(what):
        assert np.array_equal(p.mw.get_manifolds()["body"], p.w.get_manifolds()["body"]), what
        iw, is_ = p.mw.get_point_ids(), p.w.get_point_ids()
        assert iw.shape == is_.shape and np.array_equal(iw == 0, is_ == 0), what
        for x, y in zip(iw.ravel().tolist(), is_.ravel().tolist()):
            assert rename.setdefault(x, y) == y, (what, hex(x), hex(y))       # a function: a living id keeps its partner
            assert back.setdefault(y, x) == x, (what, hex(x), hex(y))         # injective
        return iw

    def step(k, what):
        for _ in range(k):
            p.step(1, what)
            ew, es = p.mw.get_contact_events(), p.w.get_contact_events()
            assert np.array_equal(_idless(ew), _idless(es)), (what, p.steps)   # no event the one context lacks, none missing
            assert _with_ids(ew, destroyed, rename) == _with_ids(es, destroyed), (what, p.steps)
            tables((what, p.steps))
            assert _with_ids(ew, created, rename) == _with_ids(es, created), (what, p.steps)

    step(40, "before")
    ids0 = tables("before the add")
    n = p.add(_spawn3())
    assert np.array_equal(tables("after the add"), ids0), "an add changes no id"
    step(25, "after the add")
    ids1 = tables("before the removal")
    victim = 1 + 64 * 4 + 5
    p.remove([victim, n + 2])
    assert np.array_equal(tables("after the removal"), ids1), "a removal changes no id (the manifolds go with the next step)"
    step(25, "after the removal")
    st = p.mw.get_edit_stats()
    assert st["shard_rebuilds"] == 0 and st["repartitions_by_edit"] == 0, st


# ---- 8. teleport and settings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_teleport_and_settings(shards):
    base = scenes.mini_piles(3, 2)
    n0 = len(base["kind"])
    s0 = _site(0, 0, 3, 2)
    scene = {k: (np.concatenate([v, _bodies([dict(pos=(s0[0] + 3.2, 0.5, s0[2]), shape=scenes.SHAPE_SPHERE, param=(0.5,))])[k]]) if isinstance(v, np.ndarray) else v)
             for k, v in base.items()}
    sphere = n0
    p = Pair(scene, shards)
    p.step(20)
    part = p.mw.get_partition()
    target = next((s for s in range(1, 6) if part[1 + 64 * s] != part[sphere]), 1)
    if shards > 1:
        assert part[1 + 64 * target] != part[sphere]
    c = _site(target % 3, target // 3, 3, 2)
    state = [a.copy() for a in p.mw.get_state()]
    state[0][sphere] = (c[0], PILE_TOP + 0.5 + 0.2, c[2]); state[2][sphere] = 0; state[3][sphere] = 0
    before = p.mw.get_edit_stats()
    p.w.set_state(*state); p.mw.set_state(*state)
    st = p.mw.get_edit_stats()
    assert st["in_place"] == before["in_place"] + 1 and st["shard_rebuilds"] == 0, st
    p.compare("after the teleport")
    p.step(30)
    assert p.mw.get_partition()[sphere] == p.mw.get_partition()[1 + 64 * target], "the sphere lives with the pile it landed on"
    p.w.set_params(gravity=(0, -4, 0), velocity_iterations=6); p.mw.set_params(gravity=(0, -4, 0), velocity_iterations=6)
    got = p.mw.get_params()
    assert got["gravity"] == (0.0, -4.0, 0.0) and got["velocity_iterations"] == 6
    ref = _capi.Params()
    assert p.w._L.edynhip_get_params(p.w._h, C.byref(ref)) == 0
    assert (got["fixed_dt"], got["position_iterations"], got["restitution_iterations"], got["individual_restitution_iterations"]) == \
        (ref.fixed_dt, ref.num_position_iterations, ref.num_restitution_iterations, ref.num_individual_restitution_iterations)
    p.step(30)
    assert p.mw.get_edit_stats()["shard_rebuilds"] == 0


# ---- 9. queries see the edit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_queries_see_the_edit(shards):
    scene = scenes.mini_piles(3, 2)
    p = Pair(scene, shards)
    p.step(30)
    n = p.add(_spawn3())
    victim = 1 + 64 * 3 + 63
    vpos = p.mw.get_state()[0][victim].copy()
    p.remove([victim])
    new = _spawn3()["pos"]
    p0 = np.concatenate([new, vpos[None]]) + np.float32([0, 30, 0])
    p1 = np.concatenate([new, vpos[None]]) - np.float32([0, 30, 0])
    hw, hs = p.mw.raycast(p0, p1), p.w.raycast(p0, p1)
    assert hw.tobytes() == hs.tobytes()
    assert hw["body"][0] == n and hw["body"][1] == n + 1 and hw["body"][3] != victim
    boxes = np.concatenate([np.concatenate([q - 0.6, q + 0.6])[None] for q in list(new) + [vpos]]).astype(np.float32)
    for cat in ("procedural", "non_procedural", "islands"):
        (ow, iw), (os_, is_) = p.mw.query_aabb(boxes, cat), p.w.query_aabb(boxes, cat)
        assert np.array_equal(ow, os_) and np.array_equal(iw, is_), cat
    ow, iw = p.mw.query_aabb(boxes, "procedural")
    assert n in iw[ow[0]:ow[1]] and n + 1 in iw[ow[1]:ow[2]] and victim not in iw
    ow, iw = p.mw.query_aabb(boxes, "non_procedural")
    assert n + 2 in iw[ow[2]:ow[3]]
    p.step(5)


# ---- 10. described, not built --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 3])
def test_edits_of_a_described_world(shards):
    scene = scenes.mini_piles(2, 1)
    extra = _bodies([dict(pos=(0.0, 6.0, 0.0), shape=scenes.SHAPE_SPHERE, param=(0.5,)),
                     dict(kind=scenes.KIND_STATIC, pos=(0.0, 0.5, 9.0), shape=scenes.SHAPE_BOX, param=(0.5, 0.5, 0.5))])
    p = Pair(scene, shards)
    n = p.add(extra)
    p.remove([7])
    assert p.mw.get_edit_stats()["edits"] == 0, "the description was edited: no shard exists yet"
    # the same scene described with the edits already made: the removed body is what its slot becomes, a shapeless static body
    made = {k: (np.concatenate([v, extra[k]]) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}
    made["kind"][7] = scenes.KIND_STATIC; made["shape_type"][7] = scenes.SHAPE_NONE
    other = MultiWorld(_cfg(), devices=[0] * shards)
    other.set_scene(made)
    live = np.ones(n + 2, bool); live[7] = False
    for _ in range(30):
        p.step(1)
        other.step_simulation(1)
        for a, b in zip(p.mw.get_state(), other.get_state()):
            assert np.array_equal(a[live], b[live]), p.steps
    assert p.mw.get_partition()[7] == -1


# ---- 11. arguments -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
def test_bad_arguments_change_nothing(shards):
    scene = scenes.c5_chains(num_chains=4, links=4)
    p = Pair(scene, shards)
    p.step(5)
    p.remove([4])                                # the last link of chain 0
    p.step(1)
    L, h = p.mw._L, p.mw._h
    n, nj = p.mw.n, p.mw.nj
    before = p.mw.get_edit_stats()
    idx = np.array([n + 5], np.uint32)
    assert L.edynhip_world_remove_bodies(h, 1, idx.ctypes.data) == ERR_INVALID
    assert b"range" in L.edynhip_world_last_error(h)
    p.step(1)
    idx = np.array([nj + 3], np.uint32)
    assert L.edynhip_world_remove_joints(h, 1, idx.ctypes.data) == ERR_INVALID
    f = np.zeros(60, np.float32)
    assert L.edynhip_world_edit_joint(h, nj + 3, f.ctypes.data, f.ctypes.data, f.ctypes.data, -1) == ERR_INVALID
    p.step(1)
    with pytest.raises(_capi.EdynHipError) as e:
        p.mw.add_joints([(scenes.JOINT_POINT, 4, 3, (0, 0, 0), (0, 0, 0), (0, 0, 1), (0, 0, 1))])
    assert e.value.code == ERR_INVALID and "removed" in str(e.value)
    with pytest.raises(_capi.EdynHipError):
        p.mw.add_joints([(scenes.JOINT_POINT, n + 1, 3, (0, 0, 0), (0, 0, 0), (0, 0, 1), (0, 0, 1))])
    assert p.mw.nj == nj
    p.step(1)
    nb, keep, b = edyn_amd.World._body_arrays(None, _bodies([dict(pos=(0, 1, 0), shape=scenes.SHAPE_SPHERE, param=(0.5,))]))
    b.pos = None
    first = C.c_uint32(0)
    assert L.edynhip_world_add_bodies(h, 1, C.byref(b), C.byref(first)) == ERR_INVALID
    assert L.edynhip_world_set_state(h, None, None, None, None) == ERR_INVALID
    assert L.edynhip_world_edit_exclusion(h, n + 1, 0, 1) == ERR_INVALID
    assert p.mw.get_edit_stats() == before and len(p.mw.get_partition()) == n
    p.step(1)


# ---- 12. a removal and a shard-rebuilding edit with no step in between -----------------------------------------------------------------
def _events_and_ids_match(p, what):
    """After a step: the id-less event rows and the id tables' shape and zero pattern equal the one context's."""
    ew, es = p.mw.get_contact_events(), p.w.get_contact_events()
    assert np.array_equal(_idless(ew), _idless(es)), what
    assert np.array_equal(p.mw.get_manifolds()["body"], p.w.get_manifolds()["body"]), what
    iw, is_ = p.mw.get_point_ids(), p.w.get_point_ids()
    assert iw.shape == is_.shape and np.array_equal(iw == 0, is_ == 0), what
    return ew


@pytest.mark.parametrize("shards", SHARDS)
def test_remove_then_capacity_fallback_without_a_step(shards):
    """The removed box's manifolds are still in its shard's context when the 400-sphere add rebuilds that shard: they travel, keep their
    ids, and the next step destroys them with the events of the one context."""
    scene = scenes.mini_piles(2, 1)
    p = Pair(scene, shards, room_bodies=420, contact_events=True)
    p.step(30)
    victim = 1 + 21
    bodies = p.mw.get_manifolds()["body"]
    assert (bodies == victim).any(), "the box is in contact"
    ids = {(int(a), int(b)): row.copy() for (a, b), row in zip(bodies, p.mw.get_point_ids())}
    p.remove([victim])
    n = p.mw.n
    grid = [dict(pos=(-19.0 + 2.0 * (k % 20), 0.3, 30.0 + 2.0 * (k // 20)), shape=scenes.SHAPE_SPHERE, param=(0.25,)) for k in range(400)]
    assert p.add(_bodies(grid)) == n
    st = p.mw.get_edit_stats()
    assert st["shard_rebuilds"] >= 1, st
    p.compare("after the removal and the add")       # the removed box's manifolds included: they go with the next step
    bodies = p.mw.get_manifolds()["body"]
    assert (bodies == victim).any()
    for (a, b), row in zip(bodies, p.mw.get_point_ids()):
        assert np.array_equal(row, ids[(int(a), int(b))]), "the rebuild changed no id"
    p.step(1)
    ev = _events_and_ids_match(p, "the step after")
    gone = ev[(ev["type"] == _capi.EVENT_MANIFOLD_DESTROYED) & ((ev["body"] == victim).any(axis=1))]
    assert len(gone) >= 1 and not (p.mw.get_manifolds()["body"] == victim).any()
    for _ in range(29):
        p.step(1)
        _events_and_ids_match(p, p.steps)


@pytest.mark.parametrize("shards", [2, 3])
def test_remove_then_bridging_spawn_without_a_step(shards):
    """A box of a pile is removed and, before any step, a beam is laid across that pile and one of another shard: the re-partition moves
    the pile with the removed box and its manifolds."""
    scene = scenes.mini_piles(3, 2)
    p = Pair(scene, shards, contact_events=True)
    p.step(20)
    part = p.mw.get_partition()
    owner = {(sx, sz): int(part[1 + 64 * (sz * 3 + sx)]) for sx in range(3) for sz in range(2)}
    pick = None
    for (sx, sz), r in sorted(owner.items()):
        for other in ((sx + 1, sz), (sx, sz + 1)):
            if pick is None and other in owner and owner[other] != r:
                pick = ((sx, sz), other)
    if pick is None:
        pytest.skip("every pair of neighbouring sites shares a shard")
    a, b = pick
    fa, fb = 1 + 64 * (a[1] * 3 + a[0]), 1 + 64 * (b[1] * 3 + b[0])
    for first in (fa, fb):                            # one box out of each of the two piles
        p.remove([first + 21])
        assert (p.mw.get_manifolds()["body"] == first + 21).any()
    ca, cb = _site(a[0], a[1], 3, 2), _site(b[0], b[1], 3, 2)
    mid = (ca + cb) / 2
    half = (5.0, 0.1, 0.3) if a[1] == b[1] else (0.3, 0.1, 5.0)
    n = p.mw.n
    p.add(_bodies([dict(pos=(mid[0], PILE_TOP + 0.11, mid[2]), shape=scenes.SHAPE_BOX, param=half)]))
    assert p.mw.get_edit_stats()["repartitions_by_edit"] >= 1
    part = p.mw.get_partition()
    assert part[fa] == part[fb] == part[n] and part[fa + 21] == part[fb + 21] == -1
    p.compare("after the removals and the beam")
    for _ in range(40):
        p.step(1)
        _events_and_ids_match(p, p.steps)
    assert not np.isin(p.mw.get_manifolds()["body"], [fa + 21, fb + 21]).any()
