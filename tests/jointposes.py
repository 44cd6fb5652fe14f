"""Joint poses at the edges of the joint rows' predicates: limits, wraps of the tracked angle, degenerate directions.

A generator in the manner of pairgen.py and bplayouts.py. cases() returns a list of named cases; a case is a dict of
  name      unique, a pytest id
  scene     2-4 amorphous bodies (no shapes, inertia diag(0.01, 0.02, 0.03) scaled by the mass) and one or two joints. The scene
            carries its settings as data, applied by apply(world, scene) to any of the three world classes:
            "hinge_params" [(joint, params10)], "joint_defs" [(joint, frameA, frameB, params16)], "generic_defs" [(joint, frameA,
            frameB, dofs[6][10])]
  steps     at most 200
  evidence  f(scene, out) that ASSERTS the edge was reached. out is what a reference run left: out["imp"] [steps, joints, 10] (nine
            applied impulses and the tracked angle), out["imp24"] [steps, joints, 24], out["state"] [steps][4]. Evidence restates a
            predicate in numpy on the start poses (for first-step edges) or reads the reference's output; it never sees the device.
  note      one line: the branch, and the number that puts the row on its true side where the pose sits exactly on a threshold

The time step is 1/60 everywhere. Unless a case says otherwise there is no gravity: the poses are exact and the speeds are chosen.
The standard pair is an anchor (body 0) at (0, 10, 0) and a link (body 1) at (0.5, 10, 0), pivots (0.25, 0, 0) / (-0.25, 0, 0).

Left out, because the reference itself does not survive them or is undefined there:
  point friction at zero relative spin   store_applied_impulses reads past its impulse array (point_constraint.cpp:55-57)
  cvjoint bend of exactly 90 degrees      |rest x twist| rounds above 1 and std::asin returns NaN
"""
import math

import numpy as np

from edyn_amd import scenes

DT = 1.0 / 60.0
PI = math.pi
KEPS = 1.1920929e-07          # EDYN_EPSILON: std::numeric_limits<float>::epsilon()
I_DIAG = (0.01, 0.02, 0.03)   # not a multiple of the identity
FAR, NEAR = (0.25, 0.0, 0.0), (-0.25, 0.0, 0.0)
X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
EYE = np.eye(3, dtype=np.float32)
S, K, D = scenes.KIND_STATIC, scenes.KIND_KINEMATIC, scenes.KIND_DYNAMIC


def frame(axis_x):
    """Orthonormal basis (row-major 3x3) whose first COLUMN is axis_x (test_reference_engine._frame)."""
    x = np.asarray(axis_x, np.float64); x = x / np.linalg.norm(x)
    y = np.cross(x, (0.0, 0.0, 1.0) if abs(x[2]) < 0.9 else (1.0, 0.0, 0.0)); y /= np.linalg.norm(y)
    z = np.cross(x, y)
    return np.stack([x, y, z], axis=1).astype(np.float32)


def quat(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([a * math.sin(angle / 2), [math.cos(angle / 2)]]).astype(np.float32)


def rotate(q, v):
    q = np.asarray(q, np.float64); v = np.asarray(v, np.float64)
    t = 2 * np.cross(q[:3], v)
    return v + q[3] * t + np.cross(q[:3], t)


def bodies(kinds, pos, mass=None, gravity=0.0):
    n = len(kinds)
    s = scenes._empty(n)
    s["kind"][:] = kinds
    s["pos"][:] = pos
    if mass is not None:
        s["mass"][:] = mass
    s["inertia"][:] = np.diag(I_DIAG).astype(np.float32).reshape(9)[None] * s["mass"][:, None]
    s["has_inertia"][:] = 1
    s["gravity"] = np.zeros((n, 3), np.float32)
    s["gravity"][:, 1] = gravity
    s["hinge_params"], s["joint_defs"], s["generic_defs"] = [], [], []
    return s


def pair(anchor=S, link_pos=(0.5, 10.0, 0.0), **kw):
    return bodies([anchor, D], [(0.0, 10.0, 0.0), link_pos], **kw)


def apply(world, scene):
    """The settings a case's scene carries, on an edyn_amd.World, the oracle or the real engine."""
    for j, p in scene.get("hinge_params", []):
        world.set_joint_params(j, p)
    for j, fa, fb, p in scene.get("joint_defs", []):
        world.set_joint_definition(j, fa, fb, p)
    for j, fa, fb, d in scene.get("generic_defs", []):
        world.set_generic_definition(j, fa, fb, d)


def merge(first, second):
    """scenes.merge, which carries "hinge_params" and "joint_defs", with the per-body gravity and the generic definitions."""
    nj = len(first["joints"])
    out = scenes.merge(first, second)
    out["gravity"] = np.concatenate([first["gravity"], second["gravity"]])
    out["generic_defs"] = list(first["generic_defs"]) + [(j + nj, fa, fb, d) for j, fa, fb, d in second["generic_defs"]]
    for k in ("joints", "hinge_params", "joint_defs"):
        out[k] = list(out[k])
    return out


def world_pivots(sc, j=0):
    """World pivots of joint j on the start poses, in float32 steps like the row preparation (rotate, then add the origin)."""
    t = sc["joints"][j]
    pA = (rotate(sc["orn"][t[1]], t[3]).astype(np.float32) + sc["pos"][t[1]]).astype(np.float32)
    pB = (rotate(sc["orn"][t[2]], t[4]).astype(np.float32) + sc["pos"][t[2]]).astype(np.float32)
    return pA, pB


# ----------------------------------------------------------------------------------------------- evidence helpers
def acted(out, col, j=0, key="imp"):
    assert np.abs(out[key][:, j, col]).max() > 0, "slot %d of joint %d never carried an impulse" % (col, j)


def silent(out, col, j=0, key="imp"):
    assert np.abs(out[key][:, j, col]).max() == 0, "slot %d of joint %d carried an impulse" % (col, j)


def first_sign(out, col, sign, j=0, key="imp"):
    v = float(out[key][0, j, col])
    assert v * sign > 0, "slot %d of joint %d after the first step: %g, wanted sign %+d" % (col, j, v, sign)


CASES = []


def case(name, steps, note):
    def deco(make):
        def build():
            sc, evidence = make()
            assert 2 <= len(sc["kind"]) <= 4 and steps <= 200 and (sc["shape_type"] == scenes.SHAPE_NONE).all()
            return dict(name=name, scene=sc, steps=steps, evidence=evidence, note=note,
                        generic=any(t[0] == scenes.JOINT_GENERIC for t in sc["joints"]))
        CASES.append(build)
        return make
    return deco


def cases():
    out = [b() for b in CASES]
    assert len({c["name"] for c in out}) == len(out)
    return out


# ----------------------------------------------------------------------------------------------- hinge
# params: angle_min, angle_max, limit_restitution, bump_stop_angle, bump_stop_stiffness, torque, speed, rest_angle, stiffness, damping
# slots:  0-2 pivot, 3-4 axis alignment, 5 limit, 6 bump stop, 7 spring, 8 torque / damping; column 9 the tracked angle
def hinge(sc, a=0, b=1, pivA=FAR, pivB=NEAR, axis=Z, params=None):
    sc["joints"].append((scenes.JOINT_HINGE, a, b, pivA, pivB, axis, axis))
    if params is not None:
        sc["hinge_params"].append((len(sc["joints"]) - 1, list(params)))
    return sc


def _wrap(rate):
    def make():
        # a kinematic body is not integrated: the anchor stays where it is, but its spin enters every row. A torque row of 10 N m
        # (0.17 N m s a step against I_zz = 0.03) brings the link to the anchor's spin within two steps, and the relative angle runs at `rate`
        sc = hinge(pair(K), pivA=(0.0, 0.0, 0.0), pivB=(0.0, 0.0, 0.0), params=[-100, 100, 0, 0, 0, 10.0, 0, 0, 0, 0])
        sc["pos"][1] = sc["pos"][0]
        sc["angvel"][0] = (0, 0, rate)

        def evidence(sc, out):
            ang = out["imp"][:, 0, 9] * (1 if rate > 0 else -1)   # grows
            assert ang[0] < 1 and ang.max() > 2 * PI + 1 and (np.diff(ang) > 0).all(), (ang[0], ang.max())   # through pi and past a whole turn, never jumping back
            assert (np.abs(ang - PI) < 0.11).any(), "no step landed next to pi"
        return sc, evidence
    return make


case("hinge_wrap_through_plus_pi", 200, "kinematic anchor at +6 rad/s: the tracked angle rises through +pi to above 2 pi")(_wrap(6.0))
case("hinge_wrap_through_minus_pi", 200, "kinematic anchor at -6 rad/s: the tracked angle falls through -pi to below -2 pi")(_wrap(-6.0))


@case("hinge_start_at_pi", 60, "link turned by exactly pi about the axis: atan2(+-0, -1), then it swings away at 1 rad/s")
def _():
    sc = hinge(pair(S, link_pos=(0.0, 10.0, 0.0)), params=[-100, 100, 0, 0, 0, 0, 0, 0, 0, 0])
    sc["orn"][1] = (0, 0, 1, 0)
    sc["angvel"][1] = (0, 0, 1.0)

    def evidence(sc, out):
        pA, pB = world_pivots(sc)
        assert np.array_equal(pA, pB) and np.array_equal(rotate(sc["orn"][1], X), (-1.0, 0.0, 0.0))
        assert abs(abs(out["imp"][0, 0, 9]) - PI) < 0.05, out["imp"][0, 0, 9]
    return sc, evidence


def _on_limit(name, lo, hi, spin, sign, note):
    @case(name, 40, note)
    def _():
        # both pivots at the centres: the pivot rows leave the spin about the axis alone
        sc = hinge(pair(S, link_pos=(0.0, 10.0, 0.0)), pivA=(0.0, 0.0, 0.0), pivB=(0.0, 0.0, 0.0), params=[lo, hi, 0, 0, 0, 0, 0, 0, 0, 0])
        sc["angvel"][1] = (0, 0, spin)

        def evidence(sc, out):
            assert (sc["orn"] == (0, 0, 0, 1)).all()   # identity orientations and equal axes: atan2(0, 1) = 0 exactly
            first_sign(out, 5, sign)
        return sc, evidence


_on_limit("hinge_on_angle_min", 0.0, 1.0, -2.0, -1, "angle 0 = angle_min, error 0; the link spins at -2 rad/s into the limit: the row pushes back (impulse < 0)")
_on_limit("hinge_on_angle_max", -1.0, 0.0, 2.0, +1, "angle 0 = angle_max, error 0; the link spins at +2 rad/s into the limit: impulse > 0")
_on_limit("hinge_on_halfway", -0.5, 0.5, 9.0, +1,
          "angle 0 = halfway: `angle < halfway` is false, the max side with error 0.5: 0.2 * 0.5 * 60 = 6 rad/s; the link spins at +9 > 6, so the max "
          "row's impulse is > 0 where the min row (taken by <=) would clamp to 0")


@case("hinge_bump_stop_left_and_entered_again", 200, "limits +-0.3 with restitution 0.9, bump stop 0.1 from each: the link bounces between them, the bump row comes and goes")
def _():
    sc = hinge(pair(S), params=[-0.3, 0.3, 0.9, 0.1, 5.0, 0, 0, 0, 0, 0])
    sc["angvel"][1] = (0, 0, 3.0)

    def evidence(sc, out):
        ang = out["imp"][:, 0, 9]
        zone = (ang < -0.2) | (ang > 0.2)   # defl != 0
        flips = np.flatnonzero(np.diff(zone.astype(int)))
        assert len(flips) >= 3, "the bump stop was not entered, left and entered again"
        acted(out, 6); acted(out, 5)
        assert zone[0] == False and (ang > 0.2).any() and (ang < -0.2).any()
    return sc, evidence


@case("hinge_spring_only", 60, "stiffness without limits: the angle is tracked, there is no limit row")
def _():
    sc = hinge(pair(S), params=[0, 0, 0, 0, 0, 0, 0, 0.3, 1.0, 0])
    sc["angvel"][1] = (0, 0, 1.0)

    def evidence(sc, out):
        acted(out, 7); silent(out, 5); silent(out, 6); silent(out, 8)
        assert np.abs(out["imp"][:, 0, 9]).max() > 0
    return sc, evidence


@case("hinge_torque_only", 60, "torque 0.05 towards speed 0.5: one row, the angle is not tracked")
def _():
    sc = hinge(pair(S), params=[0, 0, 0, 0, 0, 0.05, 0.5, 0, 0, 0])

    def evidence(sc, out):
        acted(out, 8); silent(out, 5); silent(out, 7)
        assert (out["imp"][:, 0, 9] == 0).all()
    return sc, evidence


@case("hinge_damping_only", 60, "damping without torque: the row's limits are |relative speed| * damping * dt alone")
def _():
    sc = hinge(pair(S), params=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0.05])
    sc["angvel"][1] = (0, 0, 4.0)

    def evidence(sc, out):
        acted(out, 8); silent(out, 5); silent(out, 7)
        assert abs(out["imp"][0, 0, 8]) <= 4.0 * 0.05 * DT * 1.001
    return sc, evidence


@case("hinge_min_equals_max", 60, "angle_min == angle_max = 0.2: no limit (has_limit is min < max), the torque row still acts")
def _():
    sc = hinge(pair(S), params=[0.2, 0.2, 0, 0.1, 5.0, 0.05, 0.5, 0, 0, 0])
    sc["angvel"][1] = (0, 0, 2.0)

    def evidence(sc, out):
        acted(out, 8); silent(out, 5); silent(out, 6)
    return sc, evidence


def _dyn_static(name, flip, note):
    @case(name, 60, note)
    def _():
        sc = pair(S, gravity=-9.8)
        a, b, pa, pb = (1, 0, NEAR, FAR) if flip else (0, 1, FAR, NEAR)
        hinge(sc, a, b, pa, pb, params=[-0.4, 0.4, 0.2, 0.1, 5.0, 0.01, 0.0, 0.1, 1.0, 0.02])
        sc["angvel"][1] = (0.3, 0.2, 2.0)

        def evidence(sc, out):
            t = sc["joints"][0]
            assert (sc["kind"][t[1]], sc["kind"][t[2]]) == ((D, S) if flip else (S, D))
            for c in (0, 1, 3, 5, 7, 8):
                acted(out, c)
        return sc, evidence


_dyn_static("hinge_body_a_static_b_dynamic", False, "every optional row, under gravity, bodyA static")
_dyn_static("hinge_body_a_dynamic_b_static", True, "the same joint with the bodies swapped: bodyA dynamic, bodyB static")


@case("hinge_driven_by_kinematic_anchor", 120, "the anchor stays put (a kinematic body is not integrated) but its spin of 3 rad/s enters every row, limits +-0.5 under gravity")
def _():
    sc = hinge(pair(K, gravity=-9.8), params=[-0.5, 0.5, 0.1, 0, 0, 0, 0, 0, 0, 0])
    sc["angvel"][0] = (0, 0, 3.0)

    def evidence(sc, out):
        acted(out, 5); acted(out, 0)
        assert sc["kind"][0] == K
    return sc, evidence


# ----------------------------------------------------------------------------------------------- point
@case("point_friction_spin_just_above_threshold", 40,
      "relative spin 2e-9: |w|^2 = 4e-18 > try_normalize's 1e-18; friction torque 1e-12 keeps the clamped row from stopping the spin "
      "(1.7e-12 rad/s a step). NOT zero spin: the reference reads past its impulse array there")
def _():
    sc = pair(D)
    sc["joints"].append((scenes.JOINT_POINT, 0, 1, FAR, NEAR, X, X))
    sc["hinge_params"].append((0, [1e-12]))
    sc["angvel"][1] = (0, 2e-9, 0)

    def evidence(sc, out):
        w = (sc["angvel"][0] - sc["angvel"][1]).astype(np.float32)
        l2 = float(np.float32(w @ w))
        assert 1e-18 < l2 < 1e-16
        for st in out["state"]:
            w = st[3][0] - st[3][1]
            assert 1e-18 < float(w @ w) < 1e-16   # the row was there at every step
        acted(out, 3)
    return sc, evidence


@case("point_friction_ordinary_spin", 40, "two dynamic bodies, relative spin 8 rad/s, friction torque 0.03: 0.1 rad/s a step, so the spin lasts the 40 steps")
def _():
    sc = pair(D)
    sc["joints"].append((scenes.JOINT_POINT, 0, 1, FAR, NEAR, X, X))
    sc["hinge_params"].append((0, [0.03]))
    sc["angvel"][0] = (5.0, 0, 0); sc["angvel"][1] = (-3.0, 0, 0)

    def evidence(sc, out):
        w = out["state"][-1][3]
        assert np.linalg.norm(w[0] - w[1]) > 0.1
        acted(out, 3)
    return sc, evidence


# ----------------------------------------------------------------------------------------------- distance, soft distance
def _dist(name, soft, link_x, params, vel, note, check):
    @case(name, 40, note)
    def _():
        sc = pair(S, link_pos=(link_x, 10.0, 0.0))
        sc["joints"].append((scenes.JOINT_SOFT_DISTANCE if soft else scenes.JOINT_DISTANCE, 0, 1, FAR, NEAR, X, X))
        sc["hinge_params"].append((0, list(params)))
        sc["linvel"][1] = vel

        def evidence(sc, out):
            pA, pB = world_pivots(sc)
            d = (pA - pB).astype(np.float32)
            check(sc, out, float(np.float32(d @ d)))
        return sc, evidence


def _coincident(sign):
    def check(sc, out, d2):
        assert d2 == 0.0   # !(dist_sqr > kEps): the direction falls back to (1, 0, 0)
        first_sign(out, 0, sign)
    return check


def _at_rest_length(sc, out, d2):
    assert d2 == np.float32(0.25) ** 2 and math.sqrt(d2) == 0.25
    acted(out, 0)


def _soft_at_rest(sc, out, d2):
    assert d2 == np.float32(0.25) ** 2 and math.sqrt(d2) == 0.25
    assert out["imp"][0, 0, 0] == 0 and out["imp"][0, 0, 1] != 0   # spring impulse 0: both limits 0; the damping row acts


def _soft_sign(sign, damped=True):
    def check(sc, out, d2):
        first_sign(out, 0, sign)
        acted(out, 1) if damped else silent(out, 1)
    return check


_dist("distance_pivots_coincident", False, 0.5, [0.25], (0, 0.5, 0), "separation 0, rest length 0.25: fallback direction, the row pushes the pivots apart",
      _coincident(+1))
_dist("distance_rest_length_zero", False, 0.6, [0.0], (0, 0.5, 0), "rest length 0, separation 0.1", lambda sc, out, d2: first_sign(out, 0, -1))
_dist("soft_distance_rest_length_zero", True, 0.6, [0.0, 400.0, 3.0], (0, 0.5, 0), "rest length 0, separation 0.1: spring impulse < 0", _soft_sign(-1))
_dist("distance_at_rest_length", False, 0.25, [0.25], (-1.0, 0, 0), "separation exactly the rest length 0.25: error 0; the link leaves at 1 m/s, so the row acts",
      _at_rest_length)
_dist("soft_distance_pivots_coincident", True, 0.5, [0.25, 400.0, 3.0], (0, 0.5, 0), "separation 0: fallback direction, spring impulse > 0", _coincident(+1))
_dist("soft_distance_at_rest_length", True, 0.25, [0.25, 400.0, 3.0], (-1.0, 0, 0),
      "separation exactly the rest length: spring_impulse == 0 (limits 0, error +large); the link leaves at 1 m/s, so the damping row acts", _soft_at_rest)
_dist("soft_distance_stretched", True, 0.1, [0.25, 400.0, 3.0], (-0.5, 0.2, 0), "separation 0.4 > rest length: spring impulse < 0", _soft_sign(-1))
_dist("soft_distance_compressed", True, 0.4, [0.25, 400.0, 3.0], (0.5, 0.2, 0), "separation 0.1 < rest length: spring impulse > 0", _soft_sign(+1))
_dist("soft_distance_no_damping", True, 0.1, [0.25, 400.0, 0.0], (-0.5, 0.2, 0), "damping 0: the damping row's limits are 0", _soft_sign(-1, damped=False))


# ----------------------------------------------------------------------------------------------- cone
# params: span_tan y, span_tan z, restitution, bump_stop_stiffness, bump_stop_length; slots 0 limit, 1 bump stop.
# The cone opens along +x of the anchor (frame = identity, apex at the anchor's centre); the link's pivot (0.25, 0, 0) is the point held inside.
def _cone_ps(sc):
    j, fa, fb, p = sc["joint_defs"][0]
    pA, pB = world_pivots(sc)
    pf = (pB - pA).astype(np.float32)
    return (pf * np.array([1, np.float32(1) / np.float32(p[0]), np.float32(1) / np.float32(p[1])], np.float32)).astype(np.float32)


def _cone(name, pf, spans, vel, note, check, bump=(0.0, 0.0), steps=40):
    @case(name, steps, note)
    def _():
        sc = pair(S, link_pos=(pf[0] - 0.25, 10.0 + pf[1], pf[2]))
        sc["joints"].append((scenes.JOINT_CONE, 0, 1, (0.0, 0.0, 0.0), FAR, X, X))
        sc["joint_defs"].append((0, EYE, EYE, [spans[0], spans[1], 0.1, bump[0], bump[1]]))
        sc["linvel"][1] = vel

        def evidence(sc, out):
            ps = _cone_ps(sc)
            proj = float(np.float32(ps[1] * ps[1] + ps[2] * ps[2]))
            check(ps, proj, out)
            first_sign(out, 0, +1)   # the limit row's impulse is non-zero in the reference
            acted(out, 1) if bump[0] > 0 and bump[1] > 0 else silent(out, 1)
        return sc, evidence


def _cone_on_axis(ps, proj, out):
    assert proj == 0.0 and ps[0] == 0.5


def _cone_inside(ps, proj, out):
    assert KEPS < proj < 1 and 0 < ps[0] - math.sqrt(proj) < 0.02


def _cone_on(ps, proj, out):
    n = np.array([-np.float32(math.sqrt(proj)), ps[1], ps[2]], np.float32)
    assert KEPS < proj < 1 and float(np.float32(ps @ n)) == 0.0   # error = dot(ps, normal) is exactly 0


def _cone_outside(ps, proj, out):
    assert math.sqrt(proj) > ps[0] + 0.3 and proj > KEPS


_cone("cone_pivot_on_axis", (0.5, 0.0, 0.0), (0.6, 0.9), (-6.0, 6.0, 0.0),
      "proj == 0: the fallback normal (-1, 1, 0)/sqrt 2, error -0.5/sqrt 2: 0.2 * 0.354 * 60 = 4.2 m/s; the link moves along the normal at 8.5 m/s",
      _cone_on_axis, steps=20)
_cone("cone_just_inside", (0.5, 0.29, 0.0), (0.6, 0.9), (0.0, 1.0, 0.0),
      "0.29 / 0.6 = 0.483 < 0.5, error -0.012: 0.2 * 0.012 * 60 = 0.14 m/s; the link moves outwards at 1 m/s", _cone_inside)
_cone("cone_on_the_cone", (0.5, 0.25, 0.0), (0.5, 0.9), (0.0, 1.0, 0.0), "0.25 / 0.5 = 0.5 = x exactly: error 0; the link moves outwards at 1 m/s", _cone_on)
_cone("cone_well_outside", (0.2, 0.5, 0.0), (0.6, 0.9), (0.0, 0.0, 0.3), "0.5 / 0.6 = 0.83 against x = 0.2, bump stop off (P(3) = 0)", _cone_outside)
_cone("cone_bump_stop_on", (0.2, 0.5, 0.1), (0.6, 0.9), (0.0, 0.0, 0.3), "the same with bump stop stiffness 40, length 0.1: the second row acts", _cone_outside, bump=(40.0, 0.1))
_cone("cone_bump_stop_length_zero", (0.2, 0.5, 0.1), (0.6, 0.9), (0.0, 0.0, 0.3), "stiffness 40 but length 0 (P(4) = 0): no second row",
      _cone_outside, bump=(40.0, 0.0))
_cone("cone_strongly_elliptic", (0.5, 0.3, 0.3), (0.2, 1.0), (0.0, 0.2, -0.2), "span ratio 5: scaled point (0.5, 1.5, 0.3), outside across the narrow span",
      _cone_outside)


# ----------------------------------------------------------------------------------------------- cvjoint
# params: twist_min, twist_max, twist_restitution, bump angle, bump stiffness, twist friction, twist rest angle, twist stiffness, twist damping,
#         rest direction xyz, bend stiffness, bend friction, bend damping
# slots:  0-2 pivot, 3 twist limit, 4 bump stop, 5 twist spring, 6 twist friction / damping, 7 bend friction / damping, 8 bend spring; column 9 the tracked twist
def cv(sc, fb, params, fa=EYE):
    sc["joints"].append((scenes.JOINT_CVJOINT, 0, 1, FAR, NEAR, X, X))
    sc["joint_defs"].append((len(sc["joints"]) - 1, np.asarray(fa, np.float32), np.asarray(fb, np.float32), list(params)))
    return sc


def _twist_axes(sc, j=0):
    _, fa, fb, _ = sc["joint_defs"][j]
    t = sc["joints"][j]
    return rotate(sc["orn"][t[1]], fa[:, 0]).astype(np.float32), rotate(sc["orn"][t[2]], fb[:, 0]).astype(np.float32)


CV_ALL = [-0.6, 0.8, 0.2, 0.15, 3.0, 0.01, 0.1, 2.0, 0.05, 1.0, 0.0, 0.0, 1.5, 0.02, 0.03]


@case("cvjoint_twist_axes_parallel", 60, "identity frames and orientations: shortest_arc's ordinary branch at d = 1; every optional row")
def _():
    sc = cv(pair(S), EYE, CV_ALL)
    sc["orn"][1] = quat(X, 0.75)   # a twist next to twist_max = 0.8 (a rotation about x leaves the twist axis exact)
    sc["angvel"][1] = (3.0, 0.5, 0.4)

    def evidence(sc, out):
        tA, tB = _twist_axes(sc)
        assert float(tA @ tB) == 1.0
        for c in (3, 5, 6, 7, 8):
            acted(out, c)
    return sc, evidence


@case("cvjoint_twist_axes_antiparallel", 40, "B's twist axis is -x: d = -1 <= -1 + eps, shortest_arc takes plane_space")
def _():
    sc = pair(S)
    sc["joints"].append((scenes.JOINT_CVJOINT, 0, 1, FAR, NEAR, X, X))
    sc["joint_defs"].append((0, EYE, frame((-1.0, 0.0, 0.0)), [-0.6, 0.8, 0.2, 0.15, 3.0, 0.01, 0.1, 2.0, 0.05, 1.0, 0.0, 0.0, 0.0, 0.02, 0.03]))
    sc["angvel"][1] = (2.0, 0.0, 0.0)

    def evidence(sc, out):
        tA, tB = _twist_axes(sc)
        assert float(np.float32(tA @ tB)) <= -1 + KEPS
        acted(out, 6); acted(out, 5)
    return sc, evidence


def _twist_wrap(name, rate, note):
    @case(name, 200, note)
    def _():
        # as the hinge wraps: the kinematic anchor's twist spin enters the rows, a twist friction of 10 N m brings the link to it
        sc = pair(K, link_pos=(0.0, 10.0, 0.0))
        sc["joints"].append((scenes.JOINT_CVJOINT, 0, 1, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), X, X))
        sc["joint_defs"].append((0, EYE, EYE, [-100, 100, 0, 0, 0, 10.0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]))
        sc["angvel"][0] = (rate, 0, 0)

        def evidence(sc, out):
            ang = out["imp"][:, 0, 9] * (1 if rate > 0 else -1)   # grows
            assert ang[0] < 1 and ang.max() > 2 * PI + 1 and (np.diff(ang) > 0).all(), (ang[0], ang.max())
            assert (np.abs(ang - PI) < 0.11).any(), "no step landed next to pi"
        return sc, evidence


_twist_wrap("cvjoint_twist_wrap_through_plus_pi", 6.0, "kinematic anchor with a twist spin of +6 rad/s: the tracked twist rises through +pi to above 2 pi (track_angle, in the row preparation and in the position solve)")
_twist_wrap("cvjoint_twist_wrap_through_minus_pi", -6.0, "the same at -6 rad/s: through -pi to below -2 pi")


def _bend(deg):
    @case("cvjoint_bend_%d_degrees" % deg, 30, "the link bent by %d degrees about z: bend spring at asin(sin %d), next to the 90 degrees that the reference does not survive" % (deg, deg))
    def _():
        q = quat(Z, math.radians(deg))
        link = np.asarray(FAR) - rotate(q, NEAR)
        sc = cv(pair(S, link_pos=(link[0], 10.0 + link[1], link[2])), EYE, [-0.6, 0.8, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 0.0, 1.5, 0.02, 0.0])
        sc["orn"][1] = q
        sc["angvel"][1] = (0.0, 0.0, 0.2)

        def evidence(sc, out):
            tA, tB = _twist_axes(sc)
            assert abs(math.degrees(math.acos(float(tA @ tB))) - deg) < 0.01
            acted(out, 8); acted(out, 7)
        return sc, evidence


_bend(89)
_bend(91)


def _twist_outside(name, lo, hi, spin, sign, note):
    @case(name, 40, note)
    def _():
        sc = cv(pair(S), EYE, [lo, hi, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        sc["angvel"][1] = (spin, 0, 0)

        def evidence(sc, out):
            assert (sc["orn"] == (0, 0, 0, 1)).all() and not (lo < 0.0 < hi)   # the twist angle is 0, outside the limits
            first_sign(out, 3, sign)
        return sc, evidence


_twist_outside("cvjoint_twist_below_min", 0.2, 0.8, -1.0, -1,
               "twist 0 < twist_min 0.2: the error gate is shut, rhs = -relvel alone; the link twists away at -1 rad/s so the impulse is < 0 (with the "
               "error term, 0.2 * 0.2 * 60 = 2.4 would join it)")
_twist_outside("cvjoint_twist_above_max", -0.8, -0.2, 1.0, +1, "twist 0 > twist_max -0.2: the mirror image, impulse > 0")


@case("cvjoint_no_twist_limit", 20, "twist_min >= twist_max: no twist row; the position solve corrects `current` itself - the link starts twisted by 0.1 and at rest")
def _():
    sc = cv(pair(S), EYE, [0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    sc["orn"][1] = quat(X, 0.1)

    def evidence(sc, out):
        assert (out["imp"][:, 0, 3:9] == 0).all()
        q = out["state"][0][1][1]
        assert not np.array_equal(q, sc["orn"][1]) and abs(q[0]) < abs(sc["orn"][1][0])   # only the position solve can have turned it back
    return sc, evidence


def _bend_damping(name, twist_damping, bend_damping, note):
    @case(name, 30, note)
    def _():
        sc = cv(pair(S), EYE, [-0.6, 0.8, 0, 0, 0, 0, 0, 0, twist_damping, 1.0, 0.0, 0.0, 0.0, 0.02, bend_damping])
        sc["angvel"][1] = (1.0, 0.0, 3.0)

        def evidence(sc, out):
            # a bend spin of 3 rad/s asks for far more than the friction allows: the row sits on its limit, which shows what the limit is
            lim = np.float32(0.02) * np.float32(DT)
            assert np.float32(abs(out["imp"][0, 0, 7])) == lim, (out["imp"][0, 0, 7], lim)
            acted(out, 6) if twist_damping > 0 else silent(out, 6)
        return sc, evidence


_bend_damping("cvjoint_bend_damping_without_twist_damping", 0.0, 0.05,
              "twist_damping 0, bend_damping 0.05, bend friction 0.02: the reference gates the bend damping on twist_damping, so the limit is friction * dt alone")
_bend_damping("cvjoint_twist_damping_without_bend_damping", 0.05, 0.0, "the reverse: the gate is open and adds |spin| * 0 * dt")


@case("cvjoint_bend_damping_with_twist_damping", 30, "both dampings: the bend row's limit is (friction + |bend spin| * bend_damping) * dt")
def _():
    sc = cv(pair(S), EYE, [-0.6, 0.8, 0, 0, 0, 0, 0, 0, 0.05, 1.0, 0.0, 0.0, 0.0, 0.02, 0.05])
    sc["angvel"][1] = (1.0, 0.0, 3.0)

    def evidence(sc, out):
        assert abs(out["imp"][0, 0, 7]) > 1.5 * 0.02 * DT
    return sc, evidence


@case("cvjoint_zero_bend_spin", 30, "no relative bend spin: the friction axis falls back to A's frame y; the link moves along z at 1 m/s, the pivot rows turn it about y and the row acts in the same sweep")
def _():
    sc = cv(pair(S), EYE, [-0.6, 0.8, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.02, 0.0])
    sc["linvel"][1] = (0, 0, 1.0)
    sc["angvel"][1] = (0.5, 0, 0)   # twist spin only

    def evidence(sc, out):
        tA, tB = _twist_axes(sc)
        w = [sc["angvel"][i].astype(np.float64) for i in (0, 1)]
        rel = (w[0] - (w[0] @ tA) * tA) - (w[1] - (w[1] @ tB) * tB)
        assert np.sqrt(rel @ rel) <= KEPS
        assert out["imp"][0, 0, 7] != 0
    return sc, evidence


@case("cvjoint_rest_direction_along_twist_axis", 30, "rest direction x tB = 0: the bend axis falls back to A's frame y with a bend angle, and so limits, of 0 - the row exists and can carry nothing")
def _():
    sc = cv(pair(S), EYE, [-0.6, 0.8, 0, 0, 0, 0.01, 0, 0, 0, 1.0, 0.0, 0.0, 1.5, 0.0, 0.0])
    sc["angvel"][1] = (1.0, 0, 0)

    def evidence(sc, out):
        tA, tB = _twist_axes(sc)
        assert np.linalg.norm(np.cross((1.0, 0.0, 0.0), tB)) <= KEPS
        assert out["imp"][0, 0, 8] == 0
        acted(out, 6)
    return sc, evidence


# ----------------------------------------------------------------------------------------------- generic
# dofs [6][10]: limit_enabled, min, max, restitution, bump length|angle, bump stiffness, friction, rest, spring stiffness, damping
# slot 4 * dof + {0 limit, 1 bump stop, 2 spring, 3 friction / damping}; dofs 0-2 linear along A's frame, 3 twist, 4 / 5 B's x against A's z / y
FREE, LOCKED = [0] * 10, [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def gen(sc, fb, dofs, fa=EYE, pivA=FAR, pivB=NEAR):
    sc["joints"].append((scenes.JOINT_GENERIC, 0, 1, pivA, pivB, X, X))
    sc["generic_defs"].append((len(sc["joints"]) - 1, np.asarray(fa, np.float32), np.asarray(fb, np.float32), [list(d) for d in dofs]))
    return sc


def _generic_axis(name, bx, dof, other, cos, note):
    @case(name, 30, note)
    def _():
        sc = gen(pair(S), frame(bx), [LOCKED] * 6)
        sc["angvel"][1] = (0.3, 0.2, 0.1)

        def evidence(sc, out):
            _, fa, fb, _ = sc["generic_defs"][0]
            bxw = rotate(sc["orn"][1], fb[:, 0]).astype(np.float32)
            o = np.asarray(other, np.float32)
            assert float(np.float32(bxw @ o)) == cos and not np.cross(o, bxw).any()   # cos_angle on the clamp, a null cross product: the fallback axis
            acted(out, 4 * dof, key="imp24")
        return sc, evidence


_generic_axis("generic_b_x_along_a_z", Z, 4, Z, 1.0, "cos_angle = +1 for the degree of freedom against A's z: current = pi/2 - acos(1), fallback axis (0, 0, 1); locked, so the row acts")
_generic_axis("generic_b_x_against_a_z", (0.0, 0.0, -1.0), 4, Z, -1.0, "cos_angle = -1: current = pi/2 - acos(-1)")
_generic_axis("generic_b_x_along_a_y", Y, 5, Y, 1.0, "cos_angle = +1 for the degree of freedom against A's y: fallback axis (0, 1, 0)")
_generic_axis("generic_b_x_against_a_y", (0.0, -1.0, 0.0), 5, Y, -1.0, "cos_angle = -1 against A's y")


@case("generic_twist_with_antiparallel_x", 30, "B's x is -x of A: the twist angle goes through shortest_arc's plane_space branch; twist locked")
def _():
    sc = gen(pair(S), frame((-1.0, 0.0, 0.0)), [LOCKED, LOCKED, LOCKED, LOCKED, FREE, FREE])
    sc["angvel"][1] = (2.0, 0.0, 0.0)

    def evidence(sc, out):
        _, fa, fb, _ = sc["generic_defs"][0]
        assert float(np.float32(fa[:, 0] @ fb[:, 0])) <= -1 + KEPS
        acted(out, 12, key="imp24")
    return sc, evidence


@case("generic_all_locked", 40, "six locked degrees of freedom under gravity, the link thrown")
def _():
    sc = gen(pair(S, gravity=-9.8), EYE, [LOCKED] * 6)
    sc["linvel"][1] = (0.3, 0.5, -0.4); sc["angvel"][1] = (1.0, -2.0, 0.5)

    def evidence(sc, out):
        for d in range(6):
            acted(out, 4 * d, key="imp24")
    return sc, evidence


@case("generic_all_free_friction_only", 40, "no limit anywhere, a friction row on every degree of freedom")
def _():
    fr = [0, 0, 0, 0, 0, 0, 0.02, 0, 0, 0]
    sc = gen(pair(S), EYE, [fr] * 6)
    sc["linvel"][1] = (0.3, 0.5, -0.4); sc["angvel"][1] = (1.0, -2.0, 0.5)

    def evidence(sc, out):
        for d in range(6):
            acted(out, 4 * d + 3, key="imp24"); silent(out, 4 * d, key="imp24")
    return sc, evidence


def _linear_outside(name, link_x, vel, sign, note):
    @case(name, 30, note)
    def _():
        sc = gen(pair(S, link_pos=(link_x, 10.0, 0.0)), EYE, [[1, -0.05, 0.08, 0, 0, 0, 0, 0, 0, 0], LOCKED, LOCKED, FREE, FREE, FREE])
        sc["linvel"][1] = (vel, 0, 0)

        def evidence(sc, out):
            pA, pB = world_pivots(sc)
            cur = float((pB - pA)[0])
            assert cur > 0.08 + 0.1 if sign > 0 else cur < -0.05 - 0.1
            first_sign(out, 0, sign, key="imp24")
            x = out["state"][0][0][1][0] - (sc["pos"][1][0] + np.float32(vel * DT))
            assert x * sign < 0   # the position solve pulled the link back towards the range in the first step
        return sc, evidence


_linear_outside("generic_linear_above_max", 0.7, 1.0, +1,
                "offset 0.2 > vmax 0.08: the velocity error gate is shut (with it, 0.9 * 0.12 * 60 = 6.5 m/s would swamp the link's 1 m/s outwards); the position solve pulls back")
_linear_outside("generic_linear_below_min", 0.3, -1.0, -1, "offset -0.2 < vmin -0.05: the mirror image")


@case("generic_angular_min_equals_max", 30, "vmin == vmax = 0.3 on the degree of freedom against A's y: the error is -current / dt whatever the value")
def _():
    sc = gen(pair(S), EYE, [LOCKED, LOCKED, LOCKED, FREE, FREE, [1, 0.3, 0.3, 0, 0, 0, 0, 0, 0, 0]])
    q = quat(Z, 0.2)
    link = np.asarray(FAR) - rotate(q, NEAR)
    sc["pos"][1] = (link[0], 10.0 + link[1], link[2])
    sc["orn"][1] = q

    def evidence(sc, out):
        acted(out, 20, key="imp24")
        assert out["state"][-1][1][1][2] < 0.02   # it is driven to 0, not to 0.3 (quaternion z = sin(angle / 2))
    return sc, evidence


@case("generic_spring_without_limit", 30, "limit_enabled = 0 with a spring along x, offset 0.1 from rest 0")
def _():
    sc = gen(pair(S, link_pos=(0.6, 10.0, 0.0)), EYE, [[0, 0, 0, 0, 0, 0, 0, 0.0, 50.0, 0], LOCKED, LOCKED, LOCKED, LOCKED, LOCKED])

    def evidence(sc, out):
        acted(out, 2, key="imp24"); silent(out, 0, key="imp24")
    return sc, evidence


# ----------------------------------------------------------------------------------------------- gravity
def _gravity(name, pos_b, masses, note):
    @case(name, 30, note)
    def _():
        sc = bodies([D, D], [(0.0, 10.0, 0.0), pos_b], mass=masses)
        sc["joints"].append((scenes.JOINT_GRAVITY, 0, 1, (0, 0, 0), (0, 0, 0), X, X))
        sc["linvel"][1] = (0, 0, 0.1)

        def evidence(sc, out):
            acted(out, 0)
            d = (sc["pos"][0] - sc["pos"][1]).astype(np.float32)
            assert (float(np.float32(d @ d)) <= KEPS) == (tuple(pos_b) == (0.0, 10.0, 0.0))
        return sc, evidence


_gravity("gravity_coincident_centres", (0.0, 10.0, 0.0), (2e9, 5e9), "l2 clamped to kEps")
_gravity("gravity_mass_ratio_1e6", (3.0, 10.0, 0.5), (2e9, 2e3), "masses 2e9 and 2e3")


# ----------------------------------------------------------------------------------------------- mass and inertia
@case("hinge_mass_ratio_1e6", 60, "dynamic bodies of 1e-3 and 1e3 kg (inertia scaled with them) on a limited hinge, under gravity, hung from a static anchor by a point joint")
def _():
    sc = bodies([S, D, D], [(0.0, 10.0, 0.0), (0.5, 10.0, 0.0), (1.0, 10.0, 0.0)], mass=(1.0, 1e3, 1e-3), gravity=-9.8)
    sc["joints"].append((scenes.JOINT_POINT, 0, 1, FAR, NEAR, X, X))
    hinge(sc, 1, 2, params=[-0.4, 0.4, 0.2, 0.1, 5.0, 0, 0, 0, 0, 0])
    sc["angvel"][2] = (0, 0, 3.0)

    def evidence(sc, out):
        assert abs(float(sc["mass"][1]) / float(sc["mass"][2]) / 1e6 - 1) < 1e-6
        acted(out, 5, j=1); acted(out, 0, j=1)
    return sc, evidence


@case("generic_mass_ratio_1e6", 60, "the same bodies on a generic constraint with a limited, sprung x and locked rest")
def _():
    sc = bodies([S, D, D], [(0.0, 10.0, 0.0), (0.43, 10.0, 0.0), (1.0, 10.0, 0.0)], mass=(1.0, 1e-3, 1e3), gravity=-9.8)
    sc["joints"].append((scenes.JOINT_POINT, 0, 2, (1.25, 0.0, 0.0), FAR, X, X))
    sc["joints"].append((scenes.JOINT_GENERIC, 1, 2, FAR, NEAR, X, X))
    sc["generic_defs"].append((1, EYE, EYE, [[1, -0.05, 0.08, 0.2, 0.02, 300.0, 0.01, 0.0, 50.0, 0.5], LOCKED, LOCKED, LOCKED, LOCKED, LOCKED]))
    sc["linvel"][1] = (-2.0, 0, 0)   # offset 0.07 growing by 0.033 a step: past vmax = 0.08 in the first step

    def evidence(sc, out):
        assert abs(float(sc["mass"][2]) / float(sc["mass"][1]) / 1e6 - 1) < 1e-6
        acted(out, 0, j=1, key="imp24"); acted(out, 4, j=1, key="imp24")
    return sc, evidence
