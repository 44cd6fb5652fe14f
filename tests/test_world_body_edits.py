"""Bodies of a running multi-device world edited and woken in place (edynhip_world_edit_bodies / edynhip_world_wake_bodies;
MultiWorld.edit_bodies / .wake_bodies): 1, 2 and 3 shards on device 0 against ONE context that holds the whole scene and receives the same
calls through World.edit_bodies / World.wake_bodies.

The contract: after any sequence of these calls, the other world edits and steps the world returns bit for bit what the one context
returns - state, every field of the manifolds, the sleeping tags, the multiset of contact events, queries, records - right after the call
and after EVERY step. Which path an edit took (in place, shards rebuilt because the body's kind crossed between dynamic and not dynamic,
a re-partition because the new shape reached another shard) is read from MultiWorld.get_edit_stats()."""
import ctypes as C

import numpy as np
import pytest

import edyn_amd
from edyn_amd import _capi, scenes
from edyn_amd._capi import EdynHipError
from edyn_amd.multi import MultiWorld

pytestmark = pytest.mark.gpu
SHARDS = [1, 2, 3]
DYN, KIN, STA = scenes.KIND_DYNAMIC, scenes.KIND_KINEMATIC, scenes.KIND_STATIC
BOX, SPHERE, PLANE, CYLINDER, POLY = scenes.SHAPE_BOX, scenes.SHAPE_SPHERE, scenes.SHAPE_PLANE, scenes.SHAPE_CYLINDER, scenes.SHAPE_POLYHEDRON
I_NEW = np.diag([0.3, 0.25, 0.35]).astype(np.float32).reshape(9)
I_DERIVE = np.full(9, np.nan, np.float32)
MID = 1 + 64 * 2 + 21       # a box inside the pile of site 2 (mini_piles(3, 2): the plane, then 64 boxes per site)


def _cfg(**kw):
    return edyn_amd.init_config(num_solver_velocity_iterations=10, **kw)


def _bodies(rows):
    s = scenes._empty(len(rows))
    for i, r in enumerate(rows):
        s["kind"][i] = r.get("kind", DYN)
        s["pos"][i] = r["pos"]
        s["shape_type"][i] = r["shape"]
        s["shape_param"][i, :len(r["param"])] = r["param"]
    return s


def _idless(ev):
    """The events without their ids as sorted rows (step, type, body[0], body[1])."""
    a = np.stack([ev["step"].astype(np.int64), ev["type"].astype(np.int64), ev["body"][:, 0].astype(np.int64), ev["body"][:, 1].astype(np.int64)], 1) \
        if len(ev) else np.zeros((0, 4), np.int64)
    return a[np.lexsort(a.T[::-1])]


def _apply_events(mirror, ev):
    for e in ev:
        if e["type"] == _capi.EVENT_POINT_CREATED:
            assert int(e["point_id"]) not in mirror
            mirror.add(int(e["point_id"]))
        elif e["type"] == _capi.EVENT_POINT_DESTROYED:
            mirror.remove(int(e["point_id"]))


def _touching(m, idx):
    return np.isin(m["body"], idx).any(axis=1)


class Pair:
    """The world under test and the one context it has to equal; every step is compared."""

    def __init__(self, scene, shards, room_bodies=64, room_joints=64, **kw):
        n, nj = len(scene["kind"]), len(scene.get("joints") or [])
        self.w = edyn_amd.World(_cfg(max_bodies=n + room_bodies, max_joints=nj + room_joints, **kw))
        self.w.set_scene(scene); scenes.apply_figure_settings(self.w, scene)
        self.mw = MultiWorld(_cfg(**kw), devices=[0] * shards)
        self.mw.set_scene(scene)
        self.shards = shards
        self.sleeping = bool(kw.get("sleeping"))
        self.events = bool(kw.get("contact_events"))
        self.dead = []
        self.steps = 0

    def compare(self, what=None, manifolds=True):
        what = (what, self.steps)
        assert self.mw.n == self.w.n, what
        live = np.ones(self.w.n, bool); live[self.dead] = False
        for a, b in zip(self.mw.get_state(), self.w.get_state()):
            assert np.array_equal(a[live], b[live]), what
        if manifolds:
            gm, sm = self.mw.get_manifolds(), self.w.get_manifolds()
            assert len(gm) == len(sm), what
            for f in ("body", "num_points", "colour"):
                assert np.array_equal(gm[f], sm[f]), (what, f)
            for f in _capi.POINT_DTYPE.names:
                assert np.array_equal(gm["pt"][f], sm["pt"][f]), (what, f)
        if self.sleeping:
            assert np.array_equal(self.mw.get_asleep()[live], np.asarray(self.w.get_asleep(), np.uint8)[live]), what
        if self.events:
            assert np.array_equal(_idless(self.mw.get_contact_events()), _idless(self.w.get_contact_events())), what

    def step(self, k=1, what=None, manifolds=True):
        for _ in range(k):
            self.w.step_simulation(1); self.mw.step_simulation(1)
            self.steps += 1
            self.compare(what, manifolds)

    def edit(self, idx, **kw):
        self.w.edit_bodies(idx, **kw); self.mw.edit_bodies(idx, **kw)

    def wake(self, idx):
        self.w.wake_bodies(idx); self.mw.wake_bodies(idx)

    def add(self, scene):
        fs = self.w.add_scene(scene)
        fb, fj = self.mw.add_scene(scene)
        assert fb == fs
        return fb

    def remove(self, idx):
        self.w.remove_bodies(idx); self.mw.remove_bodies(idx)
        self.dead = sorted(set(self.dead) | set(int(i) for i in idx))

    def stats_delta(self, before):
        st = self.mw.get_edit_stats()
        return {k: st[k] - before[k] for k in st}


def _in_place(delta):
    return delta["edits"] == 1 and delta["in_place"] == 1 and delta["shard_rebuilds"] == 0 and delta["repartitions_by_edit"] == 0


# ---- 1. each group alone -------------------------------------------------------------------------------------------------------------
QUIET = {
    "mass": dict(mass=[2.5]),
    "inertia_given": dict(inertia=[I_NEW]),
    "inertia_derived_with_mass": dict(mass=[0.5], inertia=[I_DERIVE]),
    "material": dict(friction=[0.9], restitution=[0.0]),
    "friction_only": dict(friction=[0.15]),
}


@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("group", list(QUIET))
def test_quiet_groups_in_place(shards, group):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    before, m0 = p.mw.get_edit_stats(), p.mw.get_manifolds()
    assert _touching(m0, [MID]).any()
    p.edit([MID], **QUIET[group])
    d = p.stats_delta(before)
    assert _in_place(d) and d["approach_checks_by_edit"] == 0, d
    m1 = p.mw.get_manifolds()
    if group in ("material", "friction_only"):      # the living points of the body's manifolds take the new friction, nothing else moves
        m0["pt"]["friction"] = m1["pt"]["friction"]
    assert m1.tobytes() == m0.tobytes(), "the call changed the manifold list"
    p.compare("after the edit")
    p.step(30)
    assert p.stats_delta(before)["shard_rebuilds"] == 0


RESHAPES = {"sphere": dict(shape_type=[SPHERE], shape_param=[(0.5, 0, 0, 0)]), "cylinder": dict(shape_type=[CYLINDER], shape_param=[(0.5, 0.5, 0, 0)])}


@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("name", list(RESHAPES))
def test_reshape_in_place(shards, name):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    before, m0 = p.mw.get_edit_stats(), p.mw.get_manifolds()
    p.edit([MID], **RESHAPES[name])
    d = p.stats_delta(before)
    assert _in_place(d) and d["approach_checks_by_edit"] == (1 if shards > 1 else 0), d
    assert p.mw.get_manifolds().tobytes() == m0[~_touching(m0, [MID])].tobytes(), "the list before minus the edited body's manifolds"
    p.compare("after the reshape")
    p.step(30)


@pytest.mark.parametrize("shards", SHARDS)
def test_replicated_plane_material_and_shape(shards):
    """Body 0, the plane every shard holds a replica of: the edit goes to every shard, no check is needed."""
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    before = p.mw.get_edit_stats()
    p.edit([0], friction=[0.2])
    d = p.stats_delta(before)
    assert _in_place(d) and d["approach_checks_by_edit"] == 0, d
    gm, sm = p.mw.get_manifolds(), p.w.get_manifolds()
    on_plane = _touching(gm, [0])
    assert on_plane.sum() >= 6 * 8 and np.array_equal(gm["pt"]["friction"], sm["pt"]["friction"])
    p.compare("plane friction")
    p.step(10)
    before = p.mw.get_edit_stats()
    p.edit([0], shape_type=[BOX], shape_param=[(40.0, 0.01, 40.0, 0)])     # a slab whose top is 1 cm above the plane
    d = p.stats_delta(before)
    assert _in_place(d) and d["approach_checks_by_edit"] == 0, d
    assert not _touching(p.mw.get_manifolds(), [0]).any()
    p.compare("plane reshaped")
    p.step(20)


# ---- 2. many at once -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_many_bodies_in_one_call(shards):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    idx = [0] + [1 + 64 * t + 37 for t in range(6)]     # the plane and a body of every pile: every shard
    before = p.mw.get_edit_stats()
    p.edit(idx, friction=np.linspace(0.2, 0.8, 7), shape_type=[BOX] + [SPHERE] * 6, shape_param=[(40.0, 0.01, 40.0, 0)] + [(0.5, 0, 0, 0)] * 6)
    assert _in_place(p.stats_delta(before))
    p.compare("seven bodies")
    p.step(15)
    n = p.mw.n
    before = p.mw.get_edit_stats()
    p.edit(np.arange(n), friction=np.full(n, 0.4), restitution=np.zeros(n))
    assert _in_place(p.stats_delta(before))
    p.compare("every body")
    p.step(15)
    p.edit(np.arange(1, n), mass=np.linspace(0.5, 2.0, n - 1), inertia=[I_DERIVE] * (n - 1))
    p.compare("every box")
    p.step(15)


# ---- 3. a reshape that reaches another shard -----------------------------------------------------------------------------------------
def _neighbour_sites(part, shards):
    """Two sites of mini_piles(3, 2) side by side, on different shards where there are several: (site, other site, axis of the step)."""
    owner = [int(part[1 + 64 * t]) for t in range(6)]
    for t in range(6):
        for u, axis in ((t + 1, 0), (t + 3, 2)):
            if u < 6 and (axis == 2 or t % 3 != 2) and (shards == 1 or owner[t] != owner[u]):
                return t, u, axis
    raise AssertionError(("no two neighbouring piles on different shards", owner))


@pytest.mark.parametrize("shards", SHARDS)
def test_reshape_that_reaches_another_shard(shards):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    t, u, axis = _neighbour_sites(p.mw.get_partition(), shards)
    pos = p.mw.get_state()[0]
    pile = np.arange(1 + 64 * t, 65 + 64 * t)
    top = int(pile[np.argmax(pos[pile, 1] * 100 + pos[pile, axis])])      # of the top layer, the box nearest to the other pile
    half = [0.5, 0.5, 0.5, 0.0]
    half[axis] = 5.0                                                        # the piles are 8 apart and 4 wide: the box ends inside the other pile's box
    before = p.mw.get_edit_stats()
    p.edit([top], shape_type=[BOX], shape_param=[half])
    d = p.stats_delta(before)
    assert d["repartitions_by_edit"] == (1 if shards > 1 else 0) and d["approach_checks_by_edit"] == (1 if shards > 1 else 0), d
    assert d["in_place"] == (0 if shards > 1 else 1), d
    part = p.mw.get_partition()
    assert part[1 + 64 * t] == part[1 + 64 * u], "the two piles share a shard now"
    p.compare("after the reshape")
    p.step(30)


# ---- 4. KIND within a class ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_plane_kinematic_and_back(shards):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    for kind in (KIN, STA):
        before = p.mw.get_edit_stats()
        p.edit([0], kind=[kind])
        d = p.stats_delta(before)
        assert _in_place(d) and d["approach_checks_by_edit"] == 0, d
        assert p.mw.get_partition()[0] == -1
        p.compare(("plane", kind))
        p.step(12)


# ---- 5. KIND crossing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_pile_box_static_and_back(shards):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(40)
    owner = int(p.mw.get_partition()[MID])
    before = p.mw.get_edit_stats()
    p.edit([MID], kind=[STA])
    d = p.stats_delta(before)
    assert d["edits"] == 1 and d["shard_rebuilds"] == shards - 1, d                 # every shard but the owner
    assert d["in_place"] == (1 if shards == 1 else 0), d
    assert p.mw.get_partition()[MID] == -1
    st = p.mw.get_state()
    assert not st[2][MID].any() and not st[3][MID].any()
    p.compare("static")
    p.step(20)                                                                       # the first of them is the warm-start proof
    before = p.mw.get_edit_stats()
    p.edit([MID], kind=[DYN], mass=[1.5], inertia=[I_NEW])
    d = p.stats_delta(before)
    assert d["shard_rebuilds"] == shards - 1 and d["in_place"] == (1 if shards == 1 else 0), d
    part = p.mw.get_partition()
    assert part[MID] >= 0 and (shards == 1 or part[MID] == part[MID + 1]), "the box lives with the pile it touches"
    assert owner >= 0
    p.compare("dynamic again")
    p.step(30)


@pytest.mark.parametrize("shards", SHARDS)
def test_falling_box_made_kinematic(shards):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(4)                                                                        # the boxes are still dropping onto each other
    assert np.abs(p.mw.get_state()[2][MID]).max() > 0
    p.edit([MID], kind=[KIN])
    assert p.mw.get_partition()[MID] == -1
    assert np.array_equal(p.mw.get_state()[2][MID], p.w.get_state()[2][MID])
    p.compare("kinematic")
    p.step(30)


def _chains_on_a_pile():
    return scenes.merge(scenes.mini_piles(2, 1), scenes.c5_chains(num_chains=4, links=8))


@pytest.mark.parametrize("shards", SHARDS)
def test_chain_link_static_and_anchor_dynamic(shards):
    scene = _chains_on_a_pile()
    n0 = 129
    p = Pair(scene, shards)
    p.step(25)
    link = n0 + 9 * 1 + 4                                                            # link 3 of chain 1
    assert any(link in (j[1], j[2]) for j in scene["joints"]) and scene["kind"][link] == DYN
    p.edit([link], kind=[STA])
    assert p.mw.get_partition()[link] == -1
    p.compare("link static")
    p.step(15)
    anchor = n0 + 9 * 2
    assert scene["kind"][anchor] == STA
    before = p.mw.get_edit_stats()
    p.edit([anchor], kind=[DYN], mass=[1.0], inertia=[np.diag([0.01, 0.01, 0.01]).astype(np.float32).reshape(9)])
    d = p.stats_delta(before)
    assert d["in_place"] == (1 if shards == 1 else 0), d
    part = p.mw.get_partition()
    assert part[anchor] >= 0 and part[anchor] == part[anchor + 1], "the anchor's joint ends on one shard"
    p.compare("anchor dynamic")
    p.step(30)


# ---- 6. sleeping ---------------------------------------------------------------------------------------------------------------------
def _asleep_pair(shards):
    scene = scenes.mini_piles(2, 1)
    p = Pair(scene, shards, sleeping=True)
    dyn = scene["kind"] == DYN
    for _ in range(16):
        p.w.step_simulation(50); p.mw.step_simulation(50)
        p.steps += 50
        if p.w.get_asleep()[dyn].all():
            break
    assert p.w.get_asleep()[dyn].all(), "the piles did not fall asleep"
    p.compare("asleep")
    return p, dyn


@pytest.mark.parametrize("shards", SHARDS)
def test_mass_wakes_nobody_shape_wakes_the_island(shards):
    p, dyn = _asleep_pair(shards)
    p.edit([1 + 21], mass=[2.0], inertia=[I_NEW])
    assert p.mw.get_asleep()[dyn].all()
    p.step(3)
    i = 1 + 21
    labels, m = p.w.get_derived()[2], p.w.get_manifolds()
    partners = set(m["body"][_touching(m, [i])].reshape(-1).tolist()) | {i}
    woken = {int(labels[b]) for b in partners if dyn[b]}
    want = dyn & np.isin(labels, list(woken))                   # the islands of the wake rule (tests/test_body_edits.py pins it on one context)
    p.edit([i], shape_type=[SPHERE], shape_param=[(0.5, 0, 0, 0)])
    awake = p.mw.get_asleep() == 0
    assert np.array_equal(awake & dyn, want) and want[i] and not awake[65:129].any(), "exactly the edited body's island and its partners'"
    p.compare("pile 0 awake")
    p.step(30)


@pytest.mark.parametrize("shards", SHARDS)
def test_wake_bodies(shards):
    p, dyn = _asleep_pair(shards)
    before = p.mw.get_edit_stats()
    labels = p.w.get_derived()[2]
    p.wake([65 + 40])
    assert _in_place(p.stats_delta(before))
    awake = p.mw.get_asleep() == 0
    assert np.array_equal(awake & dyn, dyn & (labels == labels[65 + 40])) and awake[65 + 40] and not awake[1:65].any(), "exactly the island of the body"
    p.compare("pile 1 awake")
    p.step(20)
    # an island that is awake keeps its timer: pile 1 falls asleep again on the step the one context's does, pile 0 woken now on its own
    p.wake([65 + 3, 1 + 3])
    awake = p.mw.get_asleep() == 0
    assert awake[65 + 3] and awake[1 + 3]
    p.compare("both awake")
    slept = False
    for _ in range(400):
        p.step(1, manifolds=False)
        if p.w.get_asleep()[dyn].all():
            slept = True
            break
    assert slept
    p.compare("asleep again")
    with pytest.raises(EdynHipError) as e:
        p.mw.wake_bodies([p.mw.n])
    assert e.value.code == -1
    plain = MultiWorld(_cfg(), devices=[0] * shards)      # without sleeping, or unbuilt: accepted, does nothing
    plain.set_scene(scenes.mini_piles(2, 1))
    plain.wake_bodies([3])
    plain.step_simulation(1)
    plain.wake_bodies([3])
    assert plain.get_edit_stats()["edits"] == 0


# ---- 7. events and ids ---------------------------------------------------------------------------------------------------------------
EVENT_EDITS = {
    "shape": ([MID, 0], dict(shape_type=[SPHERE, PLANE], shape_param=[(0.5, 0, 0, 0), (0, 1, 0, 0)])),
    "kind_in_class": ([0], dict(kind=[KIN])),
    "kind_crossing": ([MID, 1 + 64 * 4 + 9], dict(kind=[STA, KIN])),
}


@pytest.mark.parametrize("shards", SHARDS)
@pytest.mark.parametrize("name", list(EVENT_EDITS))
def test_events_and_ids_around_an_edit(shards, name):
    p = Pair(scenes.mini_piles(3, 2), shards, contact_events=True)
    mirror = set()

    def follow(ev):
        _apply_events(mirror, ev)
        ids = p.mw.get_point_ids()
        assert mirror == set(ids[ids != 0].tolist()), (name, p.steps)
        assert ids.shape == p.w.get_point_ids().shape

    for _ in range(25):
        p.step(1)
        follow(p.mw.get_contact_events())
    idx, kw = EVENT_EDITS[name]
    ev0, m0 = p.mw.get_contact_events(), p.mw.get_manifolds()
    seen = len(ev0)
    gone = m0[_touching(m0, idx)]
    assert len(gone) > 0
    p.edit(idx, **kw)
    ev = p.mw.get_contact_events()
    assert ev[:seen].tobytes() == ev0.tobytes(), "the last step call's events stay where they were"
    tail = ev[seen:]
    assert sorted(map(tuple, tail[tail["type"] == _capi.EVENT_MANIFOLD_DESTROYED]["body"].tolist())) == sorted(map(tuple, gone["body"].tolist()))
    assert (tail["type"] == _capi.EVENT_POINT_DESTROYED).sum() == gone["num_points"].sum()
    p.compare("right after the edit")                   # the multiset of the last step call's events plus the edit's
    follow(tail)
    for _ in range(10):
        p.step(1)
        follow(p.mw.get_contact_events())
    if name == "kind_crossing":                          # and back: the ids of everybody else's points survive the rebuilds
        seen = len(p.mw.get_contact_events())
        p.edit(idx, kind=[DYN, DYN], mass=[1.0, 1.0], inertia=[I_NEW, I_NEW])
        p.compare("dynamic again")
        assert len(p.mw.get_contact_events()) > seen, "every shard dropped its own manifolds of the two bodies"
        follow(p.mw.get_contact_events()[seen:])
        for _ in range(10):
            p.step(1)
            follow(p.mw.get_contact_events())


# ---- 8. queries and records ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_queries_and_records_see_the_edit(shards):
    p = Pair(scenes.mini_piles(3, 2), shards)
    p.step(30)
    pos = p.mw.get_state()[0]
    pile = np.arange(1 + 64 * 3, 65 + 64 * 3)
    top = int(pile[np.argmax(pos[pile, 1])])
    p0 = np.float32([pos[top] + (0, 5, 0), pos[top] + (0.42, 5, 0.42)])      # the centre, and close to a corner - where a sphere of radius 0.3 is not
    p1 = p0 - np.float32([0, 6, 0])
    assert (p.mw.raycast(p0, p1)["body"] == top).all()
    p.edit([top], shape_type=[SPHERE], shape_param=[(0.3, 0, 0, 0)])
    for bf in (False, True):
        hit = p.mw.raycast(p0, p1, brute_force=bf)
        assert hit.tobytes() == p.w.raycast(p0, p1, brute_force=bf).tobytes(), bf
        assert hit["body"][0] == top and hit["body"][1] != top
    box = np.float32([list(pos[top] - 0.45) + list(pos[top] + 0.45)])
    for a, b in zip(p.mw.query_aabb(box), p.w.query_aabb(box)):
        assert np.array_equal(a, b)
    p.step(1)
    p.w.snapshot_records(); p.mw.snapshot_records()
    rw, rs = p.mw.snapshot_map(), p.w.snapshot_map()
    assert rw[0].tobytes() == rs[0].tobytes() and rw[3] == rs[3], "records, byte for byte"
    p.step(5)


# ---- 9. composition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", SHARDS)
def test_remove_edit_and_capacity_fallback_without_a_step(shards):
    p = Pair(scenes.mini_piles(2, 1), shards, room_bodies=420, contact_events=True)
    p.step(30)
    victim, neighbour = 1 + 21, 1 + 22
    p.remove([victim])
    p.edit([neighbour], shape_type=[SPHERE], shape_param=[(0.5, 0, 0, 0)], friction=[0.3])
    p.compare("removed and edited")
    n = p.mw.n
    grid = [dict(pos=(-19.0 + 2.0 * (k % 20), 0.3, 30.0 + 2.0 * (k // 20)), shape=SPHERE, param=(0.25,)) for k in range(400)]
    assert p.add(_bodies(grid)) == n
    assert p.mw.get_edit_stats()["shard_rebuilds"] >= 1
    p.compare("and the shard rebuilt")
    p.step(30)
    p.edit([neighbour, 70], kind=[STA, STA])            # a crossing edit on the rebuilt shards
    p.compare("static after the rebuild")
    p.step(10)


@pytest.mark.parametrize("shards", [1, 3])
def test_edits_of_a_described_world(shards):
    scene = scenes.mini_piles(2, 1)
    p = Pair(scene, shards)
    p.edit([5, 70], mass=[2.0, 0.5], inertia=[I_DERIVE, I_NEW], friction=[0.8, 0.1])
    p.edit([6], shape_type=[SPHERE], shape_param=[(0.5, 0, 0, 0)])
    p.edit([100, 0], kind=[STA, KIN])
    p.edit([100], kind=[DYN], mass=[3.0], inertia=[I_NEW])
    assert p.mw.get_edit_stats()["edits"] == 0, "the description was edited: no shard exists yet"
    p.compare("described")
    p.step(30)
    assert p.mw.get_edit_stats()["shard_rebuilds"] == 0


# ---- 10. refusals change nothing -----------------------------------------------------------------------------------------------------
REFUSALS = {
    "index_out_of_range": (lambda n: dict(indices=[3, n], mass=[1.0, 1.0]), -1),
    "tombstone": (lambda n: dict(indices=[3, 60], mass=[1.0, 1.0]), -1),
    "listed_twice": (lambda n: dict(indices=[5, 9, 5], mass=[1.0, 1.0, 1.0]), -1),
    "mesh_id_that_is_no_mesh": (lambda n: dict(indices=[5], shape_type=[POLY], shape_param=[(3, 0, 0, 0)]), -1),
    "dynamic_without_mass_and_inertia": (lambda n: dict(indices=[5, 0], kind=[DYN, DYN]), -1),
}


@pytest.mark.parametrize("shards", [1, 3])
def test_refusals_change_nothing(shards):
    scene = scenes.mini_piles(2, 1)
    p = Pair(scene, shards)
    p.step(10)
    p.remove([60])
    p.step(2)
    before = p.mw.get_edit_stats()
    for name, (make, code) in REFUSALS.items():
        kw = make(p.mw.n)
        with pytest.raises(EdynHipError) as err:
            p.mw.edit_bodies(kw.pop("indices"), **kw)
        assert err.value.code == code, (name, str(err.value))
    b = _capi.Bodies()
    idx = np.array([5], np.uint32)
    assert p.mw._L.edynhip_world_edit_bodies(p.mw._h, 1, idx.ctypes.data, C.byref(b), 32) == -1      # an unknown group
    assert b"unknown field group" in p.mw._L.edynhip_world_last_error(p.mw._h)
    assert p.mw.get_edit_stats() == before
    p.compare("after the refusals")
    p.step(10)                                            # beside the one context, which never saw them
