"""Every knob-selected and size-selected kernel path against the CPU oracle, bit for bit, with evidence that the path ran.

One table, MATRIX, drives the file. A row is (knob settings, scene, steps, path bits that must be set, path bits that must stay
clear). For every row the test
  * builds the world under the row's EDYNHIP_* settings (the library reads them when the context is created, so they are set around
    World.set_scene only and removed again) - in the same process as the default world of the same scene;
  * steps it beside the oracle and compares pairs, state (as uint32) and applied joint impulses at every step, and manifolds (colours
    included) and derived state at the end; the default world of the scene went through the same comparison (its own row: no knobs),
    and the two device paths are compared with each other at every step as well. One exception, the four lattice scenes of the
    many-block colour sort, whose oracle is the slow part: oracle at steps 1, 2 and 8, the two device paths at every step;
  * asserts the row's bits of World.debug_paths() (edynhip_debug_paths: one bit per host-side branch, set at the branch), and that the
    default world's mask differs in them: none of the required bits that the row marks as the knob's own is set there, or a bit that
    must stay clear here is set there. A knob that silently selected nothing fails its row.
Everything is bit-exact: there is no tolerance in this file.

When is a knob live (DESIGN.md section 4 has the same list):
  EDYNHIP_DF_WAVES / DF_LANES    always on a contact-only scene; more than one round per wave needs na > waves * 64 / lanes
  EDYNHIP_DF_LANES=4             needs the four-lane kernel resident (df_resident[4] > 0), else it falls back to 2: the lanes bit tells
  EDYNHIP_DFP_WAVES              always on a contact-only scene; more than one round needs na > waves * 32
  EDYNHIP_DF_NAP                 a kernel argument of the two-lane velocity kernel, whenever that kernel is launched (bit: a value other than 1)
  EDYNHIP_DF_XCD                 only with a grid that is a multiple of 8 and at least 64 workgroups: na >= 2017 and DF_WAVES=64 / DFP_WAVES=64
  EDYNHIP_DATAFLOW_POS=0         contact-only scene (push schedule)
  EDYNHIP_INPLACE                only in a step whose pair set is unchanged, without contact events: a scene that has settled
  EDYNHIP_BP_ADAPT               only where the look-ahead would change: lists rebuilt four steps in a row (the host edits the state every step)
  EDYNHIP_MIXED                  joints, and at least 1 024 manifolds in islands without joints
  EDYNHIP_CC_COMPRESS            a step that relabels the islands in full; the bits count the steps whose certificate broke, not the first
  EDYNHIP_POLY_*                 polyhedron-polyhedron pairs
  EDYNHIP_WORLD_SERIAL           a world of two or more shards (one shard always runs on the caller's thread)
  direct colour sort, many blocks   more than 16 384 (17 blocks, two rows of the super table) / 32 768 manifolds

Progress of the dataflow kernels with ANY grid >= 1 (as k_contact_solve_df*, k_pos_contacts_df are written):
every wave takes its tasks in ascending sorted position p (sweep by sweep; the position kernel is one launch per iteration), the sorted
order is colour-major, and a task waits only for the previous manifold of each of its bodies in colour order - a lower p of the same
sweep - or, at a chain head, for the body's last manifold of the previous sweep. So the lowest unfinished task never waits for a higher
one, whatever the number of waves; inside a wave only the lowest pending colour is solved at a time. The XCD lists keep class (colour)
order per list. A hand-off that never arrives ends in Counters::df_abort -> EDYNHIP_ERR_INTERNAL after kDfSpinLimit polls, not in a
hang. No minimum grid: EDYNHIP_DF_WAVES=1 and EDYNHIP_DFP_WAVES=1 are run."""
import functools
import os

import numpy as np
import pytest

import edyn_amd
from edyn_amd import scenes
from edyn_amd._capi import PATH_BITS
from oracle import binding as ob
import bplayouts

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUSED = dict(fused_velocity_rows=True, block_position=True)


# ------------------------------------------------------------------ scenes
def _pile_and_ragdolls():   # the scene of test_gpu_parity.test_pile_beside_ragdolls_takes_the_mixed_schedule_bit_exact
    pile = scenes.box_pile(12, 8, 12)
    figs = scenes.figures(scenes.load_figure(os.path.join(GOLDEN, "ragdoll_capsule.npz")), 3, 2, pitch=1.6, floor=False)
    figs["pos"][:, 0] += np.float32(25.0)
    return scenes.merge(pile, figs)


def _thrown_pile():   # every body thrown about (the candidate lists are rebuilt often); the scene's `touch` steps make the look-ahead adapt
    sc = scenes.box_pile(5, 5, 5, mixed=True)
    sc["linvel"][1:] = np.random.default_rng(3).uniform(-6, 6, (125, 3)).astype(np.float32)
    return sc


def _oracle_pairs(sc):
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(sc)
    o.run_stage(0)
    return len(o.get_pairs())


@functools.lru_cache(maxsize=None)
def _tumbled_pile():
    """A 5x5x5 box pile after 110 steps of the oracle: manifolds of 1, 2, 3 and 4 points in several colours. Shared by the four
    lattice scenes, never changed."""
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    pile = scenes.box_pile(5, 5, 5)
    o.add_bodies(pile)
    o.step(110)
    for f, a in zip(("pos", "orn", "linvel", "angvel"), o.get_state()):
        pile[f] = a.copy()
    return pile


def _loose_lattice(n, target):
    """Many manifolds, cheaply: a weightless n^3 lattice of unit spheres whose AABBs overlap (26 neighbours each) but which do not
    touch - manifolds without points count towards the colour sort's M - beside a collapsed 5x5x5 box pile (several colours, all four
    point counts). target: lattice spheres are taken away from the end, then far-away pairs of spheres (one manifold each) added, until
    the first step has exactly `target` manifolds (None: as built)."""
    pile = _tumbled_pile()
    P = len(pile["kind"])

    def build(num_lattice, num_pairs):
        K = num_lattice + 2 * num_pairs
        N = P + K
        balls = scenes.subset(pile, np.ones(K, np.int64))   # K copies of a dynamic body of the pile, every field that matters set below
        for f, v in (("orn", (0, 0, 0, 1)), ("linvel", 0), ("angvel", 0), ("mass", 1), ("has_inertia", 0)):
            balls[f][:] = v
        s = scenes.merge(pile, balls)
        k, i, j = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        p = np.stack([40.0 + i.ravel() * 1.017, 20.0 + k.ravel() * 1.017, j.ravel() * 1.017], 1).astype(np.float32)[:num_lattice]
        s["pos"][P:P + num_lattice] = p
        q = np.arange(num_pairs)
        s["pos"][P + num_lattice::2] = np.stack([-40.0 - 3.0 * (q % 32), 20.0 + 3.0 * (q // 32), 0 * q], 1).astype(np.float32)
        s["pos"][P + num_lattice + 1::2] = s["pos"][P + num_lattice::2] + np.float32([1.017, 0, 0])
        s["kind"][P:] = pile["kind"][1]
        s["shape_type"][P:] = scenes.SHAPE_SPHERE
        s["shape_param"][P:] = (0.5, 0, 0, 0)
        s["gravity"] = np.tile(np.float32([0, -9.8, 0]), (N, 1))
        s["gravity"][P:] = 0
        return s
    num = n ** 3
    if target is None:
        return build(num, 0)
    while True:   # (a sphere at the end of the lattice has at most 13 neighbours before it: a step of (M - target) / 13 never overshoots)
        M = _oracle_pairs(build(num, 0))
        if M <= target:
            break
        num -= max(1, (M - target) // 13)
    sc = build(num, target - _oracle_pairs(build(num, 0)))
    assert _oracle_pairs(sc) == target
    return sc


def _blocks(lo, hi=None, exact=None):
    def check(stats_per_step, manifolds):
        M = stats_per_step[0]["num_manifolds"]
        if exact is not None:
            assert M == exact, M
        assert M > lo * 1024 and (hi is None or M <= hi * 1024), M   # the colour sort runs over more than `lo` blocks of 1 024 manifolds
        assert set(np.unique(manifolds["num_points"])) == {0, 1, 2, 3, 4}
        assert len(np.unique(manifolds["colour"][manifolds["num_points"] > 0])) >= 4
    return check


def _xcd_classes(stats_per_step, manifolds):
    act = manifolds[manifolds["num_points"] > 0]
    assert len(act) >= 2048, len(act)
    sizes = np.unique(act["colour"].astype(np.int64) * 8 + act["num_points"], return_counts=True)[1]
    assert (sizes % 32 != 0).any() and len(sizes) >= 8, sizes   # classes (colour x point count) that end inside a 32-manifold task


# name -> make the scene, solver iterations, init_config switches, the oracle's arithmetic, the steps at which the oracle is compared
# (every step, but for the four lattice scenes of the colour sort, where the oracle is the slow part: steps 1, 2 and 8, and the two
# device paths with each other at every step), a check of the scene itself (what makes the row's path live)
SCENES = {
    "mixed6": dict(make=lambda: scenes.box_pile(6, 6, 6, mixed=True)),
    "mixed6_fused_arith": dict(make=lambda: scenes.box_pile(6, 6, 6, mixed=True), cfg=FUSED, arith=ob.ARITH_FUSED_VELOCITY | ob.ARITH_BLOCK_POSITION),
    "mixed10": dict(make=lambda: scenes.box_pile(10, 10, 10, mixed=True), check=_xcd_classes),   # 9x9x9 settles at 2 039 active manifolds, 10x10x10 has 2 489 from the first step
    "mixed5": dict(make=lambda: scenes.box_pile(5, 5, 5, mixed=True)),
    # touch: the host writes the state back (unchanged) after each of these steps, as an application that steers bodies does. Every
    # such write invalidates the candidate lists, so steps 1 to 6 rebuild them: the look-ahead is halved at step 4 and again at step 5
    # (6 -> 3 -> 1.5 steps) and the thrown bodies then run on short lists, where EDYNHIP_BP_ADAPT=0 keeps the full look-ahead. (Motion
    # alone does not get there at this size: a list's slack grows with its body's speed, so only a body hit from rest outruns it.)
    "thrown5": dict(make=_thrown_pile, touch=(1, 2, 3, 4, 5)),
    "pyramid4": dict(make=lambda: scenes.pyramid(4)),
    "pyramid4_events": dict(make=lambda: scenes.pyramid(4), cfg=dict(contact_events=True), default="pyramid4"),
    "lattice17": dict(make=lambda: _loose_lattice(12, None), oracle_steps=(1, 2, 8), check=_blocks(16, 32)),
    "lattice33": dict(make=lambda: _loose_lattice(15, None), oracle_steps=(1, 2, 8), check=_blocks(32)),
    "lattice_full_blocks": dict(make=lambda: _loose_lattice(12, 17 * 1024), oracle_steps=(1, 2, 8), check=_blocks(16, 17, exact=17 * 1024)),
    "lattice_one_over": dict(make=lambda: _loose_lattice(12, 17 * 1024 + 1), oracle_steps=(1, 2, 8), check=_blocks(17, 18, exact=17 * 1024 + 1)),
    "pile_and_ragdolls": dict(make=_pile_and_ragdolls, figures=True),
    "ragdolls": dict(make=lambda: scenes.figures(scenes.load_figure(os.path.join(GOLDEN, "ragdoll_capsule.npz")), 2, 2, pitch=1.6), figures=True),   # small islands, all with joints
    "polyheap5": dict(make=lambda: scenes.polyhedron_heap(5, 5, 5)),
    # layouts of tests/bplayouts.py (held to the oracle at length in test_broadphase_edges.py): spheres in flight, whose candidate lists
    # are reused for a few steps and then expire on the device's own flag; an owner of 65 partners, one more than a lane group keeps
    "gas": dict(make=lambda: bplayouts.gas(bplayouts.GAS_CENTRES["origin"])),
    "owner65": dict(make=lambda: bplayouts.owner_k(65, speed=0.05)),
    # not stepped against the oracle's world: see _run_collide, _run_records, _run_world
    "collide_poly_poly": dict(kind="collide", shapes=(scenes.SHAPE_POLYHEDRON, scenes.SHAPE_POLYHEDRON)),
    "collide_poly_box": dict(kind="collide", shapes=(scenes.SHAPE_POLYHEDRON, scenes.SHAPE_BOX), inert=True),   # inert: the knob must select nothing here
    "records": dict(kind="records", make=lambda: scenes.box_pile(5, 5, 5, mixed=True)),
    "world_one_shard": dict(kind="world", devices=(0,), inert=True),
    "world_two_shards": dict(kind="world", devices=(0, 1)),   # (two shards on device 0 where there is no second GPU)
}

BP_ALL_OFF = {"EDYNHIP_SPECULATE": "0", "EDYNHIP_INPLACE": "0", "EDYNHIP_BP_LISTS": "0", "EDYNHIP_BP_ADAPT": "0", "EDYNHIP_DIRECT_COMPACT": "0"}
LANES = {1: "VEL_LANES1", 2: "VEL_LANES2", 4: "VEL_LANES4"}

# (knob settings, scene, steps, bits that must be set, bits that must stay clear). A required bit with a leading "=" is also set in the
# default world (the row still needs it); every other required bit must be clear there.
MATRIX = [
    # ---- the default world of every stepped scene: what the other rows are compared with, held to the oracle in the same way
    ({}, "mixed6", 60, {"=VEL_LANES2", "=COMPACT_DIRECT", "=SORT_DIRECT", "=SPECULATE", "=RELABEL_COMPRESS1"}, {"VEL_MULTI_ROUND", "POS_MULTI_ROUND", "VEL_XCD", "POS_XCD", "POS_COLOUR_PUSH", "PER_COLOUR", "VEL_NAP"}),
    ({}, "mixed6_fused_arith", 60, {"=VEL_LANES2"}, {"VEL_MULTI_ROUND", "POS_MULTI_ROUND", "POS_COLOUR_PUSH", "VEL_NAP"}),
    ({}, "mixed10", 40, {"=VEL_LANES2"}, {"VEL_XCD", "POS_XCD"}),
    ({}, "mixed5", 60, {"=COMPACT_DIRECT", "=SORT_DIRECT", "=SPECULATE"}, {"COMPACT_LIBRARY", "SORT_LIBRARY", "LISTS_FORCED"}),
    ({}, "thrown5", 60, {"=LOOKAHEAD_CHANGED"}, set()),
    ({}, "pyramid4", 30, {"=INPLACE", "=SPECULATE"}, set()),
    ({}, "lattice17", 8, {"=SORT_DIRECT"}, {"SORT_LIBRARY"}),
    ({}, "lattice33", 8, {"=SORT_DIRECT"}, {"SORT_LIBRARY"}),
    ({}, "lattice_full_blocks", 8, {"=SORT_DIRECT"}, {"SORT_LIBRARY"}),
    ({}, "lattice_one_over", 8, {"=SORT_DIRECT"}, {"SORT_LIBRARY"}),
    ({}, "pile_and_ragdolls", 30, {"=MIXED", "=PER_COLOUR"}, set()),
    ({}, "ragdolls", 30, {"=ISLAND_FUSED"}, {"MIXED", "VEL_LANES1", "VEL_LANES2", "VEL_LANES4"}),
    ({}, "polyheap5", 60, {"=POLY_AXES8", "=POLY_CONTACTS4", "=POLY_HINTS"}, {"POLY_ONE_LANE", "POLY_AXES16", "POLY_CONTACTS8", "POLY_CONTACTS16"}),
    ({}, "gas", 20, {"=LISTS_KEPT", "=LISTS_MOVED"}, {"PAIR_SURPLUS", "LISTS_FORCED"}),
    ({}, "owner65", 10, {"=PAIR_SURPLUS", "=LISTS_KEPT"}, {"LISTS_FORCED"}),
    # ---- dataflow solve
    ({"EDYNHIP_DATAFLOW_POS": "0"}, "mixed6", 60, {"POS_COLOUR_PUSH", "=VEL_LANES2"}, {"POS_MULTI_ROUND", "PER_COLOUR"}),
    ({"EDYNHIP_DATAFLOW_POS": "0"}, "mixed6_fused_arith", 60, {"POS_COLOUR_PUSH"}, set()),
] + [
    ({"EDYNHIP_DF_WAVES": str(w), "EDYNHIP_DF_LANES": str(l)}, sc, 60, {"VEL_MULTI_ROUND", ("=" if l == 2 else "") + LANES[l]}, {LANES[k] for k in LANES if k != l})
    for sc in ("mixed6", "mixed6_fused_arith") for w in (1, 3, 8) for l in (1, 2, 4)
] + [
    ({"EDYNHIP_DFP_WAVES": str(w)}, sc, 60, {"POS_MULTI_ROUND"}, {"POS_COLOUR_PUSH"}) for sc in ("mixed6", "mixed6_fused_arith") for w in (1, 3)
] + [
    # (the pause is an argument of k_contact_solve_df2, the kernel that reads it: the bit says that the launch carried another value than the default's)
    ({"EDYNHIP_DF_NAP": str(v)}, sc, 60, {"VEL_NAP", "=VEL_LANES2"}, set()) for sc in ("mixed6", "mixed6_fused_arith") for v in (0, 4)
] + [
    # ---- XCD-local task lists: 64 workgroups, classes that are no multiples of 32
    ({"EDYNHIP_DF_XCD": "1", "EDYNHIP_DF_WAVES": "64", "EDYNHIP_DFP_WAVES": "64"}, "mixed10", 40, {"VEL_XCD", "POS_XCD", "=VEL_LANES2"}, set()),
    # ---- broadphase and manifold build: collapsing pile ...
    ({"EDYNHIP_SPECULATE": "0"}, "mixed5", 60, set(), {"SPECULATE"}),
    ({"EDYNHIP_INPLACE": "0"}, "mixed5", 60, set(), {"INPLACE"}),
    ({"EDYNHIP_BP_LISTS": "0"}, "mixed5", 60, {"LISTS_FORCED"}, {"LISTS_KEPT", "LISTS_MOVED"}),
    ({"EDYNHIP_BP_ADAPT": "0"}, "mixed5", 60, set(), {"LOOKAHEAD_CHANGED"}),   # (inert here: INERT_ROWS)
    ({"EDYNHIP_DIRECT_COMPACT": "0"}, "mixed5", 60, {"COMPACT_LIBRARY"}, {"COMPACT_DIRECT"}),
    (BP_ALL_OFF, "mixed5", 60, {"LISTS_FORCED", "COMPACT_LIBRARY"}, {"SPECULATE", "COMPACT_DIRECT", "INPLACE", "LOOKAHEAD_CHANGED"}),
    # ... bodies thrown about (the look-ahead adapts) ...
    ({"EDYNHIP_BP_ADAPT": "0"}, "thrown5", 60, set(), {"LOOKAHEAD_CHANGED"}),
    (BP_ALL_OFF, "thrown5", 60, {"LISTS_FORCED", "COMPACT_LIBRARY"}, {"SPECULATE", "COMPACT_DIRECT", "INPLACE", "LOOKAHEAD_CHANGED"}),
    # ... and a scene that settles (steps in place)
    ({"EDYNHIP_INPLACE": "0"}, "pyramid4", 30, {"=SPECULATE"}, {"INPLACE"}),
    ({"EDYNHIP_SPECULATE": "0"}, "pyramid4", 30, {"=INPLACE"}, {"SPECULATE"}),
    ({"EDYNHIP_BP_LISTS": "0"}, "pyramid4", 30, {"LISTS_FORCED", "=INPLACE"}, set()),
    ({"EDYNHIP_BP_ADAPT": "0"}, "pyramid4", 30, {"=INPLACE"}, {"LOOKAHEAD_CHANGED"}),   # (inert here: INERT_ROWS)
    ({"EDYNHIP_DIRECT_COMPACT": "0"}, "pyramid4", 30, {"COMPACT_LIBRARY", "=INPLACE"}, {"COMPACT_DIRECT"}),
    (BP_ALL_OFF, "pyramid4", 30, {"LISTS_FORCED", "COMPACT_LIBRARY"}, {"SPECULATE", "COMPACT_DIRECT", "INPLACE", "LOOKAHEAD_CHANGED"}),
    ({}, "pyramid4_events", 30, {"=SPECULATE"}, {"INPLACE"}),   # contact events: no step runs in place (inplace_allowed)
    # ---- colour sort
    ({"EDYNHIP_DIRECT_SORT": "0"}, "mixed5", 60, {"SORT_LIBRARY"}, {"SORT_DIRECT"}),
    ({"EDYNHIP_DIRECT_SORT": "0"}, "lattice17", 8, {"SORT_LIBRARY"}, {"SORT_DIRECT"}),
    ({"EDYNHIP_DIRECT_SORT": "0"}, "lattice33", 8, {"SORT_LIBRARY"}, {"SORT_DIRECT"}),
    ({"EDYNHIP_DIRECT_SORT": "0"}, "lattice_full_blocks", 8, {"SORT_LIBRARY"}, {"SORT_DIRECT"}),
    ({"EDYNHIP_DIRECT_SORT": "0"}, "lattice_one_over", 8, {"SORT_LIBRARY"}, {"SORT_DIRECT"}),
    # ---- islands: rolling spheres break the certificate, so steps after the first relabel in full - the bits count those steps alone,
    # not the relabel that every freshly described scene starts with
    ({"EDYNHIP_CC_COMPRESS": "0"}, "mixed6", 60, {"RELABEL_COMPRESS0"}, {"RELABEL_COMPRESS1", "RELABEL_COMPRESSN"}),
    ({"EDYNHIP_CC_COMPRESS": "2"}, "mixed6", 60, {"RELABEL_COMPRESSN"}, {"RELABEL_COMPRESS1", "RELABEL_COMPRESS0"}),
    # ---- schedules with joints
    ({"EDYNHIP_MIXED": "0"}, "pile_and_ragdolls", 30, {"=PER_COLOUR"}, {"MIXED"}),
    ({"EDYNHIP_MIXED": "0", "EDYNHIP_ISLAND_FUSED": "0"}, "pile_and_ragdolls", 30, {"=PER_COLOUR"}, {"MIXED", "ISLAND_FUSED"}),
    ({"EDYNHIP_DATAFLOW": "0"}, "pile_and_ragdolls", 30, {"=PER_COLOUR"}, {"MIXED", "VEL_LANES2"}),   # (no dataflow launch, hence no mixed schedule)
    ({"EDYNHIP_ISLAND_FUSED": "0"}, "ragdolls", 30, {"=PER_COLOUR"}, {"ISLAND_FUSED"}),
    # ---- polyhedra
    ({"EDYNHIP_POLY_GROUP": "0"}, "polyheap5", 60, {"POLY_ONE_LANE"}, {"POLY_AXES8", "POLY_AXES16", "POLY_CONTACTS4"}),
    ({"EDYNHIP_POLY_GROUP": "16"}, "polyheap5", 60, {"POLY_AXES16", "=POLY_CONTACTS4"}, {"POLY_AXES8"}),
    ({"EDYNHIP_POLY_GROUP2": "8"}, "polyheap5", 60, {"POLY_CONTACTS8", "=POLY_AXES8"}, {"POLY_CONTACTS4"}),
    ({"EDYNHIP_POLY_GROUP2": "16"}, "polyheap5", 60, {"POLY_CONTACTS16", "=POLY_AXES8"}, {"POLY_CONTACTS4"}),
    ({"EDYNHIP_POLY_HINT": "0"}, "polyheap5", 60, {"=POLY_AXES8"}, {"POLY_HINTS"}),
    ({}, "collide_poly_poly", 0, {"=POLY_AXES8"}, {"POLY_ONE_LANE", "POLY_AXES16"}),
    ({"EDYNHIP_POLY_GROUP": "0"}, "collide_poly_poly", 0, {"POLY_ONE_LANE"}, {"POLY_AXES8", "POLY_AXES16"}),
    ({"EDYNHIP_POLY_GROUP": "16"}, "collide_poly_poly", 0, {"POLY_AXES16"}, {"POLY_AXES8", "POLY_ONE_LANE"}),
    # (a polyhedron against a box never takes the grouped kernels: the settings must change nothing, and no bit)
    ({"EDYNHIP_POLY_GROUP": "0"}, "collide_poly_box", 0, set(), {"POLY_AXES8", "POLY_AXES16", "POLY_ONE_LANE"}),
    ({"EDYNHIP_POLY_GROUP": "16"}, "collide_poly_box", 0, set(), {"POLY_AXES8", "POLY_AXES16", "POLY_ONE_LANE"}),
    # ---- records and multi-device worlds
    ({"EDYNHIP_RECORDS_DIRECT": "0"}, "records", 20, {"RECORDS_COPY"}, {"RECORDS_DIRECT"}),
    ({"EDYNHIP_RECORDS_DIRECT": "1"}, "records", 20, {"RECORDS_DIRECT"}, {"RECORDS_COPY"}),
    ({"EDYNHIP_WORLD_SERIAL": "1"}, "world_one_shard", 20, set(), {"WORLD_SERIAL"}),   # one shard always steps on the caller's thread: nothing to select
    ({"EDYNHIP_WORLD_SERIAL": "1"}, "world_two_shards", 20, {"WORLD_SERIAL"}, set()),
]


# Rows whose knob has nothing to select on their scene. They are run because every broadphase knob is run alone on both of its
# scenes; what they must show is that the knob changed nothing: the mask equals the default world's (and the result the oracle's).
INERT_ROWS = {
    # the look-ahead changes only after four list rebuilds in a row; the collapse alone never gets there at this size (thrown5 does)
    "mixed5-BP_ADAPT=0": "the look-ahead never changes in the default world of this scene",
    "pyramid4-BP_ADAPT=0": "the look-ahead never changes in the default world of this scene",
}


def _row_id(row):
    knobs, scene = row[0], row[1]
    return scene + "-" + ("default" if not knobs else "all_bp_off" if knobs is BP_ALL_OFF else
                          ",".join(k.replace("EDYNHIP_", "") + "=" + v for k, v in knobs.items()))


def knobs_in_matrix():
    return {k for row in MATRIX for k in row[0]}


def bits_required_by_matrix():
    return {b.lstrip("=") for row in MATRIX for b in row[3]}


# ------------------------------------------------------------------ the three things every row does
class _Env:
    """The row's EDYNHIP_* variables, set while the context is created and deleted again before the next world."""
    def __init__(self, monkeypatch, knobs):
        self.mp, self.knobs = monkeypatch, knobs

    def __enter__(self):
        for k in knobs_in_matrix():
            self.mp.delenv(k, raising=False)
        for k, v in self.knobs.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        for k in self.knobs:
            self.mp.delenv(k, raising=False)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]["make"]()


@functools.lru_cache(maxsize=None)
def _oracle_run(name, steps):
    """The oracle's trajectory of a scene, computed once and shared (never changed) by the scene's rows."""
    spec = SCENES[name]
    sc = _scene(name)
    ob.set_arithmetic(spec.get("arith", ob.ARITH_REFERENCE))
    try:
        o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
        o.add_bodies(sc)
        if spec.get("figures"):
            scenes.apply_figure_settings(o, sc)
        at = spec.get("oracle_steps")
        traj = {}
        for s in range(1, steps + 1):
            o.step(1)
            if s in spec.get("touch", ()):
                o.set_state(*o.get_state())
            if at is None or s in at or s == steps:
                traj[s] = (o.get_pairs().copy(), [a.copy() for a in o.get_state()], o.get_joint_impulses().copy() if sc.get("joints") else None)
        end = dict(manifolds=o.get_manifolds().copy(), derived=[a.copy() for a in o.get_derived()])
    finally:
        ob.set_arithmetic(ob.ARITH_REFERENCE)
    return traj, end


_device_runs = {}   # (scene, knobs) -> per-step state of a device world that passed its row: default and alternative are compared step by step


def _device_run(monkeypatch, name, knobs, steps):
    spec = SCENES[name]
    sc = _scene(name)
    traj, end = _oracle_run(spec.get("default", name), steps)   # (a scene that differs from another in its init_config alone shares its oracle)
    with _Env(monkeypatch, knobs):
        w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, **spec.get("cfg", {})))
        w.set_scene(sc)
        if spec.get("figures"):
            scenes.apply_figure_settings(w, sc)
    states, stats = [], []
    for s in range(1, steps + 1):
        w.step_simulation(1)
        state = w.get_state()
        states.append(state)
        if s == 1:
            stats.append(w.get_stats())
        if s in spec.get("touch", ()):
            w.set_state(*state)
        if s in traj:
            op, ostate, oimp = traj[s]
            assert np.array_equal(w.get_pairs(), op), (name, s, "pairs")
            for a, b, f in zip(state, ostate, ("pos", "orn", "linvel", "angvel")):
                assert np.array_equal(_u32(a), _u32(b)), (name, s, f)
            if oimp is not None:
                assert np.array_equal(_u32(w.get_joint_impulses()), _u32(oimp)), (name, s, "joint impulses")
    gm = w.get_manifolds()
    from test_gpu_parity import assert_manifolds_equal
    assert_manifolds_equal(gm, end["manifolds"], what=name)
    gd = w.get_derived()
    sh = sc["shape_type"] != scenes.SHAPE_NONE
    assert np.array_equal(_u32(gd[0][sh]), _u32(end["derived"][0][sh])) and np.array_equal(_u32(gd[1]), _u32(end["derived"][1])), (name, "aabb / inertia")
    assert np.array_equal(gd[2], end["derived"][2]), (name, "island labels")
    if spec.get("check"):
        spec["check"](stats, gm)
    return dict(states=states, paths=w.debug_paths())


def _default_of(monkeypatch, name, steps):
    base = SCENES[name].get("default", name)
    key = (base, steps)
    if key not in _device_runs:
        _device_runs[key] = _device_run(monkeypatch, base, {}, steps)
    return _device_runs[key]


def _assert_paths(row, paths, default_paths):
    knobs, name, _, need, clear = row
    differs = bool(knobs) or "default" in SCENES[name]
    own = {b for b in need if not b.startswith("=")}
    need = {b.lstrip("=") for b in need}
    assert need <= set(PATH_BITS) and clear <= set(PATH_BITS)
    assert need <= paths, (_row_id(row), "not taken", sorted(need - paths))
    assert not (clear & paths), (_row_id(row), "taken", sorted(clear & paths))
    if SCENES[name].get("inert") or _row_id(row) in INERT_ROWS:
        assert paths == default_paths, (_row_id(row), sorted(paths ^ default_paths))
    elif differs:   # the knob selected something: the default world's mask differs in the row's own bits
        assert not (own & default_paths), (_row_id(row), "the default world took them too", sorted(own & default_paths))
        if own or clear:
            assert own or (clear & default_paths), (_row_id(row), "the default world's mask does not differ")


def _run_stepped(monkeypatch, row):
    knobs, name, steps, _, _ = row
    default = _default_of(monkeypatch, name, steps)
    if not knobs and "default" not in SCENES[name]:
        _assert_paths(row, default["paths"], default["paths"])
        return
    alt = _device_run(monkeypatch, name, knobs, steps)
    for s, (a, b) in enumerate(zip(alt["states"], default["states"]), 1):   # the two device paths, at every step
        for x, y in zip(a, b):
            assert np.array_equal(_u32(x), _u32(y)), (_row_id(row), s)
    _assert_paths(row, alt["paths"], default["paths"])


@functools.lru_cache(maxsize=None)
def _collide_batch(shapes):
    import meshes
    from pairgen import pair_batch
    lib, rad = meshes.registered()
    st, sp, pos, orn = pair_batch(np.random.default_rng(77 + 10 * shapes[0] + shapes[1]), 20_000, shapes[0], shapes[1], rad)
    op, oc = ob.collide_batch(st, sp, pos, orn, threshold=0.02)
    return lib, (st, sp, pos, orn), (op, oc)


def _run_collide(monkeypatch, row):
    knobs, name = row[0], row[1]
    lib, batch, (op, oc) = _collide_batch(SCENES[name]["shapes"])
    masks = []
    for kn in ({}, knobs):
        with _Env(monkeypatch, kn):
            w = edyn_amd.World(edyn_amd.init_config())
            w.attach(1)
        for k, m in enumerate(lib):
            assert w.create_convex_mesh(m["vertices"], m["indices"], m["faces"]) == k
        gp, gc = w.debug_collide(*batch, threshold=0.02)
        assert np.array_equal(gc, oc) and (gc > 0).mean() > 0.5
        assert np.array_equal(_u32(gp), _u32(op))
        masks.append(w.debug_paths())
    _assert_paths(row, masks[1], masks[0])


def _run_records(monkeypatch, row):
    knobs, name, steps = row[0], row[1], row[2]
    sc = _scene(name)
    views = []
    for kn in ({}, knobs):
        with _Env(monkeypatch, kn):
            w = edyn_amd.World(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3, contact_events=True))
            w.set_scene(sc)
        w.step_simulation(steps)
        out = []
        for direct in (False, True):   # the caller's flag, which the knob overrides
            w.snapshot_records(present_dt=0.004, direct=direct)
            rec, ev, total, step = w.snapshot_map()
            assert total == len(ev) and step == steps
            out.append((rec, np.sort(ev, order=["step", "type", "body", "point_id"])))   # (the device lists a step's events in no fixed order)
        views.append((out, w.debug_paths(), w.get_state()))
    (dflt, dmask, dstate), (alt, amask, astate) = views

    def same(a, b):
        if isinstance(a, dict):
            assert a.keys() == b.keys()
            for k in a:
                same(a[k], b[k])
        elif isinstance(a, (tuple, list)):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                same(x, y)
        elif isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        else:
            assert a == b
    for v in dflt + alt:   # byte for byte, whichever way the records travelled
        same(v, dflt[0])
    assert {"RECORDS_DIRECT", "RECORDS_COPY"} <= dmask   # the default world followed the caller's flag both ways
    _assert_paths(row, amask, dmask - {"RECORDS_DIRECT", "RECORDS_COPY"})


def _run_world(monkeypatch, row):
    import torch
    knobs, name, steps = row[0], row[1], row[2]
    devices = tuple(d if d < torch.cuda.device_count() else 0 for d in SCENES[name]["devices"])
    from edyn_amd.multi import MultiWorld
    sc = scenes.mini_piles(3, 2)
    res = []
    for kn in ({}, knobs):
        with _Env(monkeypatch, kn):
            w = MultiWorld(edyn_amd.init_config(num_solver_velocity_iterations=10, num_solver_position_iterations=3), devices=devices)
            w.set_scene(sc)
            w.step_simulation(1)   # (the shards' contexts are created by the first step)
        w.step_simulation(steps - 1)
        res.append((w.get_state(), w.get_manifolds(), w.debug_paths()))
        w.close()
    (ds, dm, dmask), (as_, am, amask) = res
    for x, y in zip(ds, as_):
        assert np.array_equal(_u32(x), _u32(y))
    assert dm.tobytes() == am.tobytes() and len(dm) > 0
    traj, _ = _world_oracle(steps)
    for x, y in zip(as_, traj):
        assert np.array_equal(_u32(x), _u32(y))
    _assert_paths(row, amask, dmask)


@functools.lru_cache(maxsize=None)
def _world_oracle(steps):
    o = ob.World(vel_iters=10, pos_iters=3, order=ob.ORDER_COLOURED)
    o.add_bodies(scenes.mini_piles(3, 2))
    o.step(steps)
    return [a.copy() for a in o.get_state()], None


@pytest.mark.parametrize("row", MATRIX, ids=[_row_id(r) for r in MATRIX])
def test_knob_path_bit_exact_and_taken(monkeypatch, row):
    kind = SCENES[row[1]].get("kind", "stepped")
    {"stepped": _run_stepped, "collide": _run_collide, "records": _run_records, "world": _run_world}[kind](monkeypatch, row)
