"""Bodies of a running world edited in place (edynhip_edit_bodies / World.edit_bodies): mass, inertia, material, shape, kind.

The yardstick is a TWIN, built from public calls after the edit: a fresh World from the edited description - with the edited world's
get_state() as its poses and velocities -, the same joints, materials and mix table, set_manifolds(get_manifolds()),
set_joint_warm_start, set_asleep and set_sleep_timers. Edited world and twin must then agree bit for bit: AABBs and world inverse
inertias right away (the island labels of a fresh world are recomputed by its first step, so they are compared from the first step
on), and state, manifold records (order, colours, lifetimes, impulses), joint impulses, sleeping flags, pair keys, AABBs, inertias and
labels after each of 30 steps. Every dynamic body carries an explicit inertia, as the C++ shim gives it, so that a SHAPE edit leaves
nothing to derive; one case derives the inertia (has_inertia 0, centre-of-mass offset included).
Two cases are also held to the CPU oracle, and the call itself is checked without a step: what leaves the manifold array, what
friction the points take, who wakes, what a ray sees, which events arrive, and what is refused.
"""
import ctypes as C
import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes, _capi
from edyn_amd._capi import EdynHipError
from edyn_amd.multi import MultiWorld
from oracle import binding as ob

pytestmark = pytest.mark.gpu

DYN, KIN, STA = scenes.KIND_DYNAMIC, 1, scenes.KIND_STATIC
BOX, SPHERE, PLANE, CYLINDER, POLY = scenes.SHAPE_BOX, scenes.SHAPE_SPHERE, scenes.SHAPE_PLANE, 5, scenes.SHAPE_POLYHEDRON
STEPS = 30
I_NEW = np.diag([0.3, 0.25, 0.2]).astype(np.float32).reshape(9)


# ------------------------------------------------------------------ scenes
def _copy(scene):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in scene.items()}


def _explicit_inertia(scene):
    """Every dynamic body that has none gets an inertia of its own (mass / 6 on the diagonal: the unit cube's)."""
    s = _copy(scene)
    need = (s["kind"] == DYN) & (s["has_inertia"] == 0)
    s["inertia"][need] = np.outer(s["mass"][need] / np.float32(6), np.eye(3, dtype=np.float32).reshape(9))
    s["has_inertia"][need] = 1
    return s


def _with_loner(scene):
    """One more dynamic box far from everything: a body without manifolds (it is still falling when the test ends)."""
    extra = scenes._empty(1)
    extra["shape_type"][0] = BOX
    extra["shape_param"][0, :3] = 0.5
    extra["pos"][0] = (40.0, 60.0, 40.0)
    out = scenes.merge(scene, extra)
    for k in ("hinge_params", "joint_defs", "exclusions"):
        out.pop(k)
    if "meshes" in scene:
        out["meshes"] = scene["meshes"]
    return out


def pile_scene():
    return _explicit_inertia(_with_loner(scenes.box_pile(6, 6, 6)))   # ~1000 manifolds once settled: several workgroups of the compaction


def mixed_scene():
    return _explicit_inertia(scenes.box_pile(5, 5, 5, mixed=True))


def heap_scene():
    return _explicit_inertia(scenes.polyhedron_heap(3, 3, 2, pitch=1.1))


def chain_scene():
    """Four chains of four links (point and hinge joints alternating) hanging from static anchors just above a 4x4x4 pile and coming
    to rest on it; the links are spheres."""
    chains = scenes.c5_chains(4, 4)
    chains["pos"][:, 0] -= 1.0
    chains["pos"][:, 1] -= 5.2
    chains["pos"][:, 2] -= 1.0
    link = chains["kind"] == DYN
    chains["shape_type"][link] = SPHERE
    chains["shape_param"][link] = (0.2, 0, 0, 0)
    out = scenes.merge(scenes.box_pile(4, 4, 4), chains)
    for k in ("hinge_params", "joint_defs", "exclusions"):
        out.pop(k)
    return _explicit_inertia(out)


def sleep_scene():
    """Four separate 4x4x4 piles and a pair of boxes on the ground held together by a point joint: five islands that all fall asleep."""
    pair = scenes._empty(2)
    pair["shape_type"][:] = BOX
    pair["shape_param"][:, :3] = 0.5
    pair["pos"][:] = ((20.0, 0.505, 0.0), (21.5, 0.505, 0.0))
    pair["joints"] = [(scenes.JOINT_POINT, 0, 1, (0.75, 0, 0), (-0.75, 0, 0), (1, 0, 0), (1, 0, 0))]
    out = scenes.merge(scenes.mini_piles(2, 2), pair)
    for k in ("hinge_params", "joint_defs", "exclusions"):
        out.pop(k)
    out["sleeping_disabled"] = np.zeros(len(out["kind"]), np.uint8)
    return _explicit_inertia(out)


# ------------------------------------------------------------------ worlds, twins, comparisons
def make_world(scene, setup=None, **cfg):
    w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, **cfg))
    w.set_scene(scene)
    if setup:
        setup(w)
    return w


def edited_description(scene, idx, mass=None, inertia=None, friction=None, restitution=None, shape_type=None, shape_param=None, kind=None):
    """The scene description after the edit, one value (or one row) per entry of idx. A row of NaN in `inertia`: derived."""
    s = _copy(scene)
    idx = np.asarray(idx)
    if mass is not None:
        s["mass"][idx] = mass
    if inertia is not None:
        I = np.broadcast_to(np.asarray(inertia, np.float32).reshape(-1, 9), (len(idx), 9))
        given = ~np.isnan(I).any(axis=1)
        s["inertia"][idx] = np.nan_to_num(I)
        s["has_inertia"][idx] = given
    if friction is not None:
        s["friction"][idx] = friction
    if restitution is not None:
        s["restitution"][idx] = restitution
    if shape_type is not None:
        s["shape_type"][idx] = shape_type
        s["shape_param"][idx] = np.asarray(shape_param, np.float32).reshape(-1, 4)
    if kind is not None:
        s["kind"][idx] = kind
    return s


def twin_of(w, scene, setup=None, **cfg):
    s = _copy(scene)
    s["pos"], s["orn"], s["linvel"], s["angvel"] = w.get_state()
    t = make_world(s, setup, **cfg)
    t.set_state(*w.get_state())
    t.set_manifolds(w.get_manifolds())
    if w.nj:
        t.set_joint_warm_start(w.get_joint_impulses24(), w.get_joint_impulses()[:, 9])
    if cfg.get("sleeping"):
        t.set_asleep(w.get_asleep())
        t.set_sleep_timers(*w.get_sleep_timers())
    return t


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_derived_equal(a, b, scene, what, labels=True):
    da, db = a.get_derived(), b.get_derived()
    sh = scene["shape_type"] != scenes.SHAPE_NONE
    assert same_bits(da[0][sh], db[0][sh]), (what, "aabb", np.flatnonzero((da[0] != db[0]).any(axis=1)))
    assert same_bits(da[1], db[1]), (what, "world inverse inertia", np.flatnonzero((da[1] != db[1]).any(axis=1)))
    if labels:
        assert same_bits(da[2], db[2]), (what, "island labels")


def assert_worlds_equal(a, b, what):
    for x, y, f in zip(a.get_state(), b.get_state(), ("pos", "orn", "linvel", "angvel")):
        assert same_bits(x, y), (what, f, np.flatnonzero((x != y).any(axis=1)))
    ma, mb = a.get_manifolds(), b.get_manifolds()
    assert len(ma) == len(mb), (what, "manifold count", len(ma), len(mb))
    assert same_bits(ma, mb), (what, "manifold records", np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(ma, mb)])[:8])
    assert same_bits(a.get_joint_impulses24(), b.get_joint_impulses24()), (what, "joint impulses")
    assert same_bits(a.get_asleep(), b.get_asleep()), (what, "sleeping flags")
    assert same_bits(a.get_pairs(), b.get_pairs()), (what, "pair keys")


def lockstep(a, b, scene, what, steps=STEPS):
    for s in range(steps):
        a.step_simulation(1); b.step_simulation(1)
        assert_worlds_equal(a, b, (what, "step", s))
        assert_derived_equal(a, b, scene, (what, "step", s))


def check_against_twin(w, scene_after, what, setup=None, **cfg):
    t = twin_of(w, scene_after, setup, **cfg)
    assert_derived_equal(w, t, scene_after, (what, "right away"), labels=False)
    assert_worlds_equal(w, t, (what, "right away"))
    lockstep(w, t, scene_after, what)


def owners_of(w, scene):
    """The bodies that own the first and the last manifold of the sorted array (the dynamic body, the higher index of two)."""
    m = w.get_manifolds()
    def owner(r):
        a, b = int(r["body"][0]), int(r["body"][1])
        da, db = scene["kind"][a] == DYN, scene["kind"][b] == DYN
        return max(a, b) if da and db else (a if da else b)
    return sorted({owner(m[0]), owner(m[-1])})


def touching(m, idx):
    return np.isin(m["body"][:, 0], idx) | np.isin(m["body"][:, 1], idx)


# ------------------------------------------------------------------ the edit lists and the groups
def pile_lists(w, scene):
    n = len(scene["kind"])
    return {"one": [100], "no_manifold": [n - 1], "first_last": owners_of(w, scene), "plane": [0], "all": list(range(n))}


def group_edit(group, scene, idx):
    """The arguments of edit_bodies for one group over the bodies idx: the plane stays a static plane, everybody else changes."""
    idx = np.asarray(idx)
    plane = scene["shape_type"][idx] == PLANE
    n = len(idx)
    kw = {}
    if group in ("mass", "combo"):
        kw["mass"] = np.full(n, 2.5, np.float32)
    if group in ("inertia", "combo"):
        kw["inertia"] = np.tile(I_NEW, (n, 1))
    if group == "material":
        kw["friction"] = np.full(n, 0.8, np.float32)
    if group in ("shape", "combo"):
        kw["shape_type"] = np.where(plane, PLANE, SPHERE).astype(np.int32)
        sp = np.tile(np.float32([0.45, 0, 0, 0]), (n, 1))
        sp[plane] = (0, 1, 0, 0)
        kw["shape_param"] = sp
    if group == "kind":
        kw["kind"] = np.where(plane, STA, KIN).astype(np.int32)
    if group == "combo":
        kw["kind"] = np.where(plane, STA, DYN).astype(np.int32)
    return kw


@pytest.mark.parametrize("which", ["one", "no_manifold", "first_last", "plane", "all"])
@pytest.mark.parametrize("group", ["mass", "inertia", "material", "shape", "kind", "combo"])
def test_each_group_on_the_box_pile(group, which):
    """box_pile(6, 6, 6) settled for 25 steps: each group alone, and SHAPE + KIND + MASS + INERTIA in one call, over one body, a body
    without manifolds, the owners of the first and the last manifold, the static plane (every ground manifold goes with SHAPE / KIND)
    and every body at once; then 30 steps beside the twin."""
    scene = pile_scene()
    w = make_world(scene)
    w.step_simulation(25)
    idx = pile_lists(w, scene)[which]
    before = w.get_manifolds()
    assert len(before) > 4 * 256
    kw = group_edit(group, scene, idx)
    w.edit_bodies(idx, **kw)
    after = w.get_manifolds()
    if group in ("shape", "kind", "combo"):   # the manifolds of the edited bodies, and only they, left the array
        assert same_bits(after, before[~touching(before, idx)]), (group, which)
        if which != "no_manifold":
            assert len(after) < len(before)
    elif group != "material":
        assert same_bits(after, before), (group, which)
    check_against_twin(w, edited_description(scene, idx, **kw), (group, which))


def test_null_edit_changes_nothing():
    """MASS, INERTIA and MATERIAL with the values the bodies already have: the edited world goes on bit for bit like an untouched copy
    stepped beside it, and keeps its candidate lists and its manifold array (the paths an untouched world takes)."""
    scene = pile_scene()
    a, b = make_world(scene), make_world(scene)
    a.step_simulation(25); b.step_simulation(25)
    idx = np.arange(len(scene["kind"]))
    a.edit_bodies(idx, mass=scene["mass"], inertia=scene["inertia"], friction=scene["friction"], restitution=scene["restitution"])
    assert_worlds_equal(a, b, "null edit, right away")
    assert_derived_equal(a, b, scene, "null edit, right away")
    lockstep(a, b, scene, "null edit")
    assert a.debug_paths() == b.debug_paths()


def test_derived_inertia_with_centre_of_mass_offset():
    """MASS + INERTIA with has_inertia 0: the inertia comes from the body's shape, the new mass and its centre-of-mass offset, as an
    upload derives it. Edited before the first step, so that the twin's description holds the very origins the world was given."""
    scene = scenes.box_pile(3, 3, 3)   # (no explicit inertias here)
    scene["com"] = np.zeros((len(scene["kind"]), 3), np.float32)
    scene["com"][5] = (0.1, -0.05, 0.2)
    scene["com"][9] = (0.0, 0.15, 0.0)
    idx = [5, 9, 12]
    w = make_world(scene)
    kw = dict(mass=np.float32([3.0, 0.5, 2.0]), inertia=np.full((3, 9), np.nan, np.float32))
    w.edit_bodies(idx, **kw)
    t = make_world(edited_description(scene, idx, **kw))
    assert_derived_equal(w, t, scene, "derived inertia, right away")
    lockstep(w, t, scene, "derived inertia")


@pytest.mark.parametrize("name", ["sphere_to_box_in_the_mixed_pile", "box_to_cylinder", "box_to_new_polyhedron", "polyhedron_to_box", "chain_link_to_box"])
def test_shape_changes(name):
    setup = None
    if name == "sphere_to_box_in_the_mixed_pile":
        scene = mixed_scene()
        i = int(np.flatnonzero(scene["shape_type"] == SPHERE)[20])
        kw = dict(shape_type=[BOX], shape_param=[(0.4, 0.5, 0.45, 0)])
    elif name == "box_to_cylinder":   # a world that had no cylinder: the narrowphase's cylinder kernel comes on
        scene, i = pile_scene(), 130
        kw = dict(shape_type=[CYLINDER], shape_param=[(0.45, 0.5, 1, 0)])
    elif name == "box_to_new_polyhedron":   # a mesh created after the bodies went up; the world held no polyhedron before
        scene, i = pile_scene(), 130
        kw = dict(shape_type=[POLY], shape_param=[(0, 0, 0, 0)])
    elif name == "polyhedron_to_box":
        scene, i = heap_scene(), 7
        kw = dict(shape_type=[BOX], shape_param=[(0.4, 0.4, 0.4, 0)])
    else:
        scene = chain_scene()
        i = len(scene["kind"]) - 2
        kw = dict(shape_type=[BOX], shape_param=[(0.2, 0.15, 0.2, 0)])
    w = make_world(scene)
    w.step_simulation(60 if name in ("polyhedron_to_box", "chain_link_to_box") else 25)
    after = edited_description(scene, [i], **kw)
    if name == "box_to_new_polyhedron":
        mesh = scenes.convex_library()[3]
        assert w.create_convex_mesh(mesh["vertices"], mesh["indices"], mesh["faces"]) == 0
        after["meshes"] = [mesh]
    before = w.get_manifolds()
    assert touching(before, [i]).any()
    w.edit_bodies([i], **kw)
    assert same_bits(w.get_manifolds(), before[~touching(before, [i])])
    check_against_twin(w, after, name, setup)


def test_dynamic_to_kinematic_and_back():
    scene = pile_scene()
    i = 140
    w = make_world(scene)
    w.step_simulation(25)
    w.edit_bodies([i], kind=[KIN])
    kin = edited_description(scene, [i], kind=[KIN])
    t = twin_of(w, kin)
    assert_derived_equal(w, t, kin, "kinematic, right away", labels=False)
    lockstep(w, t, kin, "kinematic", steps=8)
    back = dict(kind=[DYN], mass=[1.5], inertia=[I_NEW])
    w.edit_bodies([i], **back)
    check_against_twin(w, edited_description(kin, [i], **back), "dynamic again")


def test_dynamic_to_static():
    scene = pile_scene()
    w = make_world(scene)
    w.step_simulation(25)
    idx = [30, 141]
    w.edit_bodies(idx, kind=[STA, STA])
    st = w.get_state()
    assert not st[2][idx].any() and not st[3][idx].any()
    check_against_twin(w, edited_description(scene, idx, kind=[STA, STA]), "static")


def test_chain_link_made_static():
    """A link of a hinge chain becomes static: its joints are coloured again (a joint end that is not dynamic constrains nothing) and
    keep their applied impulses."""
    scene = chain_scene()
    w = make_world(scene)
    w.step_simulation(60)
    i = len(scene["kind"]) - 3
    assert any(i in (j[1], j[2]) for j in scene["joints"])
    w.edit_bodies([i], kind=[STA])
    check_against_twin(w, edited_description(scene, [i], kind=[STA]), "chain link static")


def test_mass_edit_on_the_chains():
    scene = chain_scene()
    w = make_world(scene)
    w.step_simulation(60)
    idx = [len(scene["kind"]) - 1, 20]
    kw = dict(mass=[0.4, 3.0], inertia=[I_NEW, I_NEW])
    w.edit_bodies(idx, **kw)
    check_against_twin(w, edited_description(scene, idx, **kw), "chains, mass and inertia")


# ------------------------------------------------------------------ the call itself
_probe_cache = {}


def created_friction(fa, fb):
    """The friction the device gives a point it creates between materials fa and fb: a box dropped onto a plane, one step."""
    key = (float(fa), float(fb))
    if key not in _probe_cache:
        s = scenes.box_pile(1, 1, 1)
        s["friction"][:] = (fb, fa)
        p = make_world(s)
        p.step_simulation(1)
        m = p.get_manifolds()
        assert len(m) == 1 and m["num_points"][0] > 0
        _probe_cache[key] = np.float32(m["pt"]["friction"][0, 0])
    return _probe_cache[key]


def test_material_edit_sets_the_points_friction():
    """No step: the manifold list is the list before, with every living point of the edited bodies' manifolds at the friction the
    device mixes for a new point of the two materials; a pair the mix table combines keeps its friction; restitution reaches new
    points only and turns the restitution pass on for them."""
    scene = pile_scene()
    tabled = 1   # body 1 rests on the plane: the pair (body 1, plane) is combined by the mix table

    def setup(w):
        w.set_material_ids(0, [7])
        w.set_material_ids(tabled, [9])
        w.insert_material_mixing(9, 7, restitution=0.0, friction=0.33)

    w = make_world(scene, setup)
    w.step_simulation(25)
    before = w.get_manifolds()
    idx = [tabled, 100]
    w.edit_bodies(idx, friction=[0.8, 0.2], restitution=[0.25, 0.0])
    after = w.get_manifolds()
    fric = np.asarray(scene["friction"]).copy()
    fric[idx] = (0.8, 0.2)
    want = before.copy()
    seen_tabled = seen_mixed = 0
    for r in want:
        a, b = int(r["body"][0]), int(r["body"][1])
        if a not in idx and b not in idx:
            continue
        if {a, b} == {0, tabled}:
            assert np.all(r["pt"]["friction"][:r["num_points"]] == np.float32(0.33))
            seen_tabled += 1
            continue
        r["pt"]["friction"][:r["num_points"]] = created_friction(fric[a], fric[b])
        seen_mixed += int(r["num_points"])
    assert seen_tabled == 1 and seen_mixed > 8
    assert same_bits(after, want)
    assert not same_bits(after, before)
    check_against_twin(w, edited_description(scene, idx, friction=[0.8, 0.2], restitution=[0.25, 0.0]), "material", setup)


def test_partial_material_arguments_keep_the_other_coefficient():
    scene = pile_scene()
    scene["restitution"][50] = 0.125
    w = make_world(scene)
    w.step_simulation(5)
    w.edit_bodies([50], friction=[0.7])
    w.edit_bodies([51], restitution=[0.3])
    check_against_twin(w, edited_description(edited_description(scene, [50], friction=[0.7]), [51], restitution=[0.3]), "partial material")


def _asleep_world():
    scene = sleep_scene()
    w = make_world(scene, sleeping=True)
    for _ in range(12):
        w.step_simulation(50)
        if w.get_asleep()[scene["kind"] == DYN].all():
            break
    assert w.get_asleep()[scene["kind"] == DYN].all(), "the piles did not fall asleep"
    return scene, w


@pytest.mark.parametrize("which", ["pile_body", "jointed_box", "plane"])
def test_shape_edit_wakes_exactly_the_islands_of_the_rule(which):
    """Sleeping scene, every island asleep. After a SHAPE edit exactly these are awake: the islands of the edited bodies, of the
    bodies that shared a dropped manifold with them, of the bodies that share a joint with them. Then 30 steps beside the twin."""
    scene, w = _asleep_world()
    n = len(scene["kind"])
    labels = w.get_derived()[2]
    i = {"pile_body": 70, "jointed_box": n - 1, "plane": 0}[which]
    m = w.get_manifolds()
    partners = set(m["body"][touching(m, [i])].reshape(-1).tolist()) | {i}
    partners |= {b for j in scene["joints"] if i in (j[1], j[2]) for b in (j[1], j[2])}
    woken = {int(labels[b]) for b in partners if scene["kind"][b] == DYN}
    want = np.array([scene["kind"][b] == DYN and int(labels[b]) in woken for b in range(n)])
    assert want.any() and (which == "plane" or not want[scene["kind"] == DYN].all())
    kw = dict(shape_type=[PLANE], shape_param=[(0, 1, 0, 0)]) if which == "plane" else dict(shape_type=[SPHERE], shape_param=[(0.5, 0, 0, 0)])
    w.edit_bodies([i], **kw)
    assert np.array_equal(~w.get_asleep() & (scene["kind"] == DYN), want)
    lab, since, _ = w.get_sleep_timers()
    assert all(since[l] < 0 for l in woken), "the woken islands' timers restart"
    check_against_twin(w, edited_description(scene, [i], **kw), ("wake", which), sleeping=True)


def test_mass_edit_wakes_nobody():
    scene, w = _asleep_world()
    idx = [70, len(scene["kind"]) - 1]
    kw = dict(mass=[2.0, 2.0], inertia=[I_NEW, I_NEW], friction=[0.9, 0.9])
    w.edit_bodies(idx, **kw)
    assert w.get_asleep()[scene["kind"] == DYN].all()
    before = w.get_state()
    w.step_simulation(3)
    assert all(same_bits(x, y) for x, y in zip(before, w.get_state()))
    assert w.get_asleep()[scene["kind"] == DYN].all()


def test_raycast_sees_the_new_shape_before_any_step():
    scene = pile_scene()
    w = make_world(scene)
    w.step_simulation(25)
    pos = w.get_state()[0]
    top = int(np.argmax(np.where(np.arange(len(pos)) < len(pos) - 1, pos[:, 1], -1)))   # a box of the top layer (not the loner)
    # rays straight down onto the box: its centre, and close to a corner - where a sphere of radius 0.3 is not
    p0 = np.float32([pos[top] + (0, 5, 0), pos[top] + (0.42, 5, 0.42)])
    p1 = p0 - np.float32([0, 6, 0])
    hit_box = [w.raycast(p0, p1, brute_force=bf) for bf in (False, True)]
    assert same_bits(hit_box[0], hit_box[1]) and (hit_box[0]["body"] == top).all()
    kw = dict(shape_type=[SPHERE], shape_param=[(0.3, 0, 0, 0)])
    w.edit_bodies([top], **kw)
    hit = [w.raycast(p0, p1, brute_force=bf) for bf in (False, True)]
    assert same_bits(hit[0], hit[1])
    assert hit[0]["body"][0] == top and hit[0]["body"][1] != top
    assert hit[0]["fraction"][0] > hit_box[0]["fraction"][0]   # the sphere's top is 0.2 below the box's
    t = twin_of(w, edited_description(scene, [top], **kw))
    for bf in (False, True):
        assert same_bits(t.raycast(p0, p1, brute_force=bf), hit[0])


def _apply_events(mirror, ev):
    for e in ev:
        if e["type"] == _capi.EVENT_POINT_CREATED:
            assert int(e["point_id"]) not in mirror
            mirror.add(int(e["point_id"]))
        elif e["type"] == _capi.EVENT_POINT_DESTROYED:
            mirror.remove(int(e["point_id"]))


@pytest.mark.parametrize("group", ["shape", "kind", "material"])
def test_event_stream_keeps_a_mirror_in_step(group):
    """With contact_events a mirror fed by the event stream alone holds exactly get_point_ids(): after the settling steps, after the
    edit - whose events are appended to the list of the last step call - and after each of 10 further steps. Every dropped manifold
    is reported destroyed, once."""
    scene = pile_scene()
    w = make_world(scene, contact_events=True)
    mirror = set()
    for _ in range(25):
        w.step_simulation(1)
        _apply_events(mirror, w.get_contact_events())
    ids = w.get_point_ids()
    assert mirror == set(ids[ids != 0].tolist())
    idx = [0, 100] if group == "shape" else [100, 101, 150]
    seen = len(w.get_contact_events())
    before = w.get_manifolds()
    w.edit_bodies(idx, **group_edit(group, scene, idx))
    ev = w.get_contact_events()[seen:]
    gone = before[touching(before, idx)]
    if group == "material":
        assert len(ev) == 0
    else:
        destroyed = ev[ev["type"] == _capi.EVENT_MANIFOLD_DESTROYED]
        assert sorted(map(tuple, destroyed["body"].tolist())) == sorted(map(tuple, gone["body"].tolist()))
        assert (ev["type"] == _capi.EVENT_POINT_DESTROYED).sum() == gone["num_points"].sum()
        assert set(np.unique(ev["type"]).tolist()) <= {_capi.EVENT_MANIFOLD_DESTROYED, _capi.EVENT_POINT_DESTROYED}
    _apply_events(mirror, ev)
    ids = w.get_point_ids()
    assert mirror == set(ids[ids != 0].tolist())
    for s in range(10):
        w.step_simulation(1)
        _apply_events(mirror, w.get_contact_events())
        ids = w.get_point_ids()
        assert mirror == set(ids[ids != 0].tolist()), s


REFUSALS = {
    "index_out_of_range": (lambda n: dict(indices=[3, n], mass=[1.0, 1.0]), -1),
    "removed_body": (lambda n: dict(indices=[60], mass=[1.0]), -1),
    "listed_twice": (lambda n: dict(indices=[5, 9, 5], mass=[1.0, 1.0, 1.0]), -1),
    "shape_none": (lambda n: dict(indices=[5], shape_type=[scenes.SHAPE_NONE], shape_param=[(0, 0, 0, 0)]), -6),
    "shape_beyond_polyhedron": (lambda n: dict(indices=[5], shape_type=[7], shape_param=[(0, 0, 0, 0)]), -6),
    "mesh_id_that_is_no_mesh": (lambda n: dict(indices=[5], shape_type=[POLY], shape_param=[(3, 0, 0, 0)]), -1),
    "dynamic_without_mass_and_inertia": (lambda n: dict(indices=[5], kind=[DYN]), -1),
    "derived_inertia_without_mass": (lambda n: dict(indices=[5], inertia=[np.full(9, np.nan)]), -1),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_the_world_as_it_was(name):
    """Every refusal is decided before anything changes: a list with a valid first entry is refused as a whole, and the next step is
    bit for bit the step of an untouched copy."""
    scene = pile_scene()
    a, b = make_world(scene), make_world(scene)
    for w in (a, b):
        w.step_simulation(10)
        w.remove_bodies([60])
        w.step_simulation(2)
    make, code = REFUSALS[name]
    kw = make(len(scene["kind"]))
    with pytest.raises(EdynHipError) as err:
        a.edit_bodies(kw.pop("indices"), **kw)
    assert err.value.code == code, str(err.value)
    assert_worlds_equal(a, b, (name, "right away"))
    assert_derived_equal(a, b, scene, (name, "right away"))
    lockstep(a, b, scene, name, steps=2)


def test_empty_edit_is_valid():
    scene = pile_scene()
    a, b = make_world(scene), make_world(scene)
    a.step_simulation(5); b.step_simulation(5)
    a.edit_bodies([], mass=[], kind=[])
    lockstep(a, b, scene, "n == 0", steps=2)


def test_shard_of_a_multi_device_world_is_refused():
    mw = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10), devices=(0,))
    mw.set_scene(scenes.box_pile(2, 2, 2))
    mw._L.edynhip_world_context.restype = C.c_void_p
    ctx = C.c_void_p(mw._L.edynhip_world_context(mw._h, 0))
    idx = np.uint32([1])
    mass = np.float32([2.0])
    values = _capi.Bodies()
    values.mass = mass.ctypes.data_as(C.c_void_p)
    assert mw._L.edynhip_edit_bodies(ctx, 1, idx.ctypes.data_as(C.c_void_p), C.byref(values), _capi.EDIT_MASS) == -6   # EDYNHIP_ERR_UNSUPPORTED
    mw.close()


# ------------------------------------------------------------------ an independent check: the CPU oracle
@pytest.mark.parametrize("group", ["mass", "shape"])
def test_edited_pile_steps_like_the_oracle(group):
    """box_pile(6, 6, 6), sleeping off: after the edit an oracle world of the edited description takes the device's state, manifolds
    and joint warm start, and both step 10 times in lock-step (coloured order): pair keys, state and manifolds bit for bit."""
    from test_gpu_parity import assert_manifolds_equal   # every field of the living points, as that file compares with the oracle
    scene = pile_scene()
    w = make_world(scene)
    w.step_simulation(25)
    idx = [100, 101, 150, 37]
    kw = group_edit(group, scene, idx)
    w.edit_bodies(idx, **kw)
    after = edited_description(scene, idx, **kw)
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(after)
    o.set_state(*w.get_state())
    o.refresh_derived()
    o.set_manifolds(w.get_manifolds())
    for s in range(10):
        w.step_simulation(1); o.step(1)
        assert np.array_equal(w.get_pairs(), o.get_pairs()), (group, s)
        for x, y, f in zip(w.get_state(), o.get_state(), ("pos", "orn", "linvel", "angvel")):
            assert same_bits(x, y), (group, s, f)
        assert_manifolds_equal(w.get_manifolds(), o.get_manifolds(), what=(group, s))
