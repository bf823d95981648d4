"""Capsules as link collision shapes (include/bioik_hip.h: CAPSULES) under ClearanceGoal (opcode 19), SelfClearanceGoal (opcode 20) and TouchGoal (opcode 17) on the
library under test: the GPU suite (tests/test_gpu_capsules.py) and the host simulator (tests/test_hostsim_capsules.py) run these cases.  `make_solver(template)`
makes a bio_ik_amd.solver.HipSolver of the library under test.

THE PIN is the cost restated in long double from the header alone, out of pieces that exist and are imported as they are: the long-double forward kinematics of
tests/np_fk.py, base_link_cases.relative / relative_bound for opcode 20's frame R, and clearance_cases.clearance for the point-against-point pairs.  New here are
the two distances, in long double and taken ROBUSTLY rather than by the device's formula:

    point against segment     t = clamp(e.u / u.u, 0, 1) (0 where u.u == 0),  |e - t u|            the formula is exact in exact arithmetic
    segment against segment   min( the four end-against-segment distances,  the distance of the two lines' closest points where both parameters lie in (0, 1) )

(the minimum of a convex function over the unit square is attained in its interior, where the gradient vanishes, or on an edge, where one end is held; exactly
parallel axes have no interior candidate and need none).  Not the oracle (it does not know the opcodes) and not the kernel.

THE BOUND.  The check is error <= bound, the bound derived here, not tuned; -s prints the worst error / bound ratio.  Per pair of primitives the device's
penetration pen = max(0, s - d) is off by at most

    e = d_p + (rot + C U) vmax + C U (|s| + omax + amax) + kappa                         pen^2: random_robot_cases.sq_bound(pen, e), summed, times weight^2

with C, U, the frame bounds d_p / d_q and rot = 2 d_q (1 + |q|^2) exactly as tests/clearance_cases.py has them for a sphere centre.  Two facts carry it.
First, the inputs: the distance from a point to a segment, and between two segments, is 1-Lipschitz in every end and in the point (moving an end by delta moves
every point of the segment by at most delta).  So a carried-over end enters exactly as a sphere centre does: vmax is the larger of the two ends' norms in the
link frame (|v_i| for a point), amax the larger norm of the carried-over ends, omax that of the other primitive's rows.  Second, the arithmetic: the device's
distance is the distance of two points that LIE ON the segments, so it can exceed the true minimum only through the error of its parameters.  For a point against
a segment the parameter is one well-conditioned quotient and the distance is stationary in it (or the clamp is exact): second order, inside the C U term.  For two
segments the first parameter is s = (u.v v.w - v.v u.w) / (u.u v.v - (u.v)^2), and its denominator is u.u v.v sin^2(theta), theta the angle between the axes: it
cancels.  Numerator and denominator carry a few U of |u| |v|^2 |w| and of u.u v.v, so

    |ds| <= C U (1 + |w| / min(|u|, |v|)) / sin^2(theta),        and never more than 1 (s is clamped)

t follows from s by a well-conditioned quotient and is clamped exactly; where it leaves [0, 1] the device solves s again exactly for the clamped end.  Moving along
one axis by ds |u| changes the distance to the other axis' line by that times sin(theta) -- so

    kappa = (|u| + |v|) min( sin(theta),  C U (1 + |w| / min(|u|, |v|)) / sin(theta) )       0 for sin(theta) == 0, and for a point against anything

computed in long double from the inputs.  It peaks near sin(theta) = sqrt(C U ...), about 1e-7: a few 1e-8 m on 0.3 m segments (a float64 prototype of the device's
formula against long double measured 6.8e-9 m on 1e5 pairs 1e-12 ... 1e-1 rad from parallel, 1.9e-16 m on random pairs).  Exactly parallel axes -- and axes that
are parallel up to the rounding of a rotation, sin(theta) about 1e-16 -- meet the ordinary bound: any s gives the same distance there.
The running sum rounds once per pair that adds something: (C + pairs) U cost on top, as in tests/clearance_cases.py."""
import functools
import os
import types

import numpy as np

import base_link_cases as bl
import clearance_cases as cc
import np_goals
import random_robot_cases as rr
import self_clearance_cases as sc
import touch_cases as tc
from bio_ik_amd import ClearanceGoal, PoseGoal, PositionGoal, ProblemTemplate, SelfClearanceGoal, TouchGoal, abi, pr2_like
from bio_ik_amd.robot import link_transform
from np_fk import LD
from tools import record_clearance_bits

C, U = rr.C, rr.U
RW, LW, RE, LE, RF, LF = sc.RW, sc.LW, sc.RE, sc.LE, sc.RF, sc.LF
TIP = cc.TIP
PAD = "r_pad"  # a link fixed to the right wrist with an identity rotation: R = inv(wrist) o pad is the same translation for every individual
PAD_AT = (0.1, 0.0, 0.0)
CLEAR, SELF = abi.GOAL_CLEARANCE, abi.GOAL_SELF_CLEARANCE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clearance_parent_bits.npz")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a * b).sum(axis=-1)


def norm(a):
    return np.sqrt(dot(a, a))


def point_segment(A, B, c):
    """distance of c from the segment A B (arrays (..., 3), long double); a segment of length 0 is its first end"""
    u, e = B - A, c - A
    uu = dot(u, u)
    t = np.where(uu > 0, np.clip(dot(e, u) / np.where(uu > 0, uu, LD(1)), LD(0), LD(1)), LD(0))
    return norm(e - t[..., None] * u)


def segment_segment(A, B, Cc, D):
    """distance of the segments A B and Cc D: the least of the four end-against-segment distances and the interior candidate"""
    best = np.minimum(np.minimum(point_segment(Cc, D, A), point_segment(Cc, D, B)), np.minimum(point_segment(A, B, Cc), point_segment(A, B, D)))
    u, v, w = B - A, D - Cc, A - Cc
    a, b, c, d, e = dot(u, u), dot(u, v), dot(v, v), dot(u, w), dot(v, w)
    den = a * c - b * b
    ok = den > 0
    safe = np.where(ok, den, LD(1))
    s, t = (b * e - c * d) / safe, (a * e - b * d) / safe
    ok = ok & (s > 0) & (s < 1) & (t > 0) & (t < 1)
    inner = norm(w + s[..., None] * u - t[..., None] * v)
    return np.minimum(best, np.where(ok, inner, LD(np.inf)))


def kappa(A, B, Cc, D):
    """the conditioning term of a segment pair (module docstring), float64 from long-double inputs"""
    u, v, w = B - A, D - Cc, A - Cc
    nu, nv, nw = norm(u), norm(v), norm(w)
    ok = (nu > 0) & (nv > 0)
    sin = np.where(ok, norm(np.cross(u, v)) / np.where(ok, nu * nv, LD(1)), LD(0))
    pos = sin > 0
    cond = LD(C * U) * (1 + nw / np.where(ok, np.minimum(nu, nv), LD(1))) / np.where(pos, sin, LD(1))
    return np.asarray(np.where(pos, (nu + nv) * np.minimum(sin, cond), LD(0)), dtype=np.float64)


def carried(p, q, rows):
    """(n, rows, 3): p + rotate(q, v) for the rows' xyz (long double), q as it is"""
    rows = np.asarray(rows, dtype=LD).reshape(-1, 3)
    if rows.shape[0] == 0:
        return np.zeros((np.asarray(p).shape[0], 0, 3), dtype=LD)
    return np.stack([np.asarray(p, dtype=LD) + tc.rotate_ld(q, r) for r in rows], axis=1)


def capsule_pairs(margin, p, q, pts, caps, obs, ocaps, d_p, d_q):
    """every pair that involves a capsule -- the link's points (n_p, 4) and capsules (k, 8) carried over by (p, q) (n individuals), against the other side's points
    (m, 4) and capsules (k', 8) as they are: (cost (n,) long double, bound (n,), deepest penetration (n,), least gap d - radii (n,))"""
    n = np.asarray(p).shape[0]
    pts, caps, obs, ocaps = (np.asarray(a, dtype=LD).reshape(-1, w) for a, w in ((pts, 4), (caps, 8), (obs, 4), (ocaps, 8)))
    f64 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    qn = np.linalg.norm(f64(q), axis=1)
    rot = (2 * d_q * (1 + qn * qn))[:, None, None]
    dp = np.asarray(d_p, dtype=np.float64)[:, None, None]
    cost, bound, deep, gap, pairs = np.zeros(n, dtype=LD), np.zeros(n), np.zeros(n), np.full(n, np.inf), 0
    W = carried(p, q, pts[:, :3])                                            # (n, n_p, 3)
    A, B = carried(p, q, caps[:, :3]), carried(p, q, caps[:, 4:7])           # (n, k, 3)
    blocks = []
    if pts.shape[0] and ocaps.shape[0]:    # L's points against O's capsules
        d = point_segment(ocaps[None, None, :, :3], ocaps[None, None, :, 4:7], W[:, :, None, :])
        blocks.append((d, (LD(margin) + pts[:, 3])[:, None] + ocaps[None, :, 3], pts[:, 3][:, None] + ocaps[None, :, 3], f64(norm(pts[:, :3]))[None, :, None], f64(norm(W))[:, :, None],
                       f64(np.maximum(norm(ocaps[:, :3]), norm(ocaps[:, 4:7])))[None, None, :], 0.0))
    if caps.shape[0]:
        vmax = f64(np.maximum(norm(caps[:, :3]), norm(caps[:, 4:7])))[None, :, None]
        amax = f64(np.maximum(norm(A), norm(B)))[:, :, None]
        if obs.shape[0]:                   # L's capsules against O's points
            d = point_segment(A[:, :, None, :], B[:, :, None, :], obs[None, None, :, :3])
            blocks.append((d, (LD(margin) + caps[:, 3])[:, None] + obs[None, :, 3], caps[:, 3][:, None] + obs[None, :, 3], vmax, amax, f64(norm(obs[:, :3]))[None, None, :], 0.0))
        if ocaps.shape[0]:                 # L's capsules against O's capsules
            a4 = (A[:, :, None, :], B[:, :, None, :], ocaps[None, None, :, :3], ocaps[None, None, :, 4:7])
            blocks.append((segment_segment(*a4), (LD(margin) + caps[:, 3])[:, None] + ocaps[None, :, 3], caps[:, 3][:, None] + ocaps[None, :, 3], vmax, amax,
                           f64(np.maximum(norm(ocaps[:, :3]), norm(ocaps[:, 4:7])))[None, None, :], kappa(*a4)))
    for d, s, radii, vmax, amax, omax, kap in blocks:
        pen = np.where(s[None] > 0, np.maximum(LD(0), s[None] - d), LD(0))
        e = dp + (rot + C * U) * vmax + C * U * (np.abs(f64(s))[None] + omax + amax) + kap
        cost = cost + (pen * pen).sum(axis=(1, 2))
        bound = bound + rr.sq_bound(f64(pen), e).sum(axis=(1, 2))
        deep = np.maximum(deep, f64(pen).max(axis=(1, 2)))
        gap = np.minimum(gap, f64(d - radii[None]).min(axis=(1, 2)))
        pairs += pen.shape[1] * pen.shape[2]
    return cost, bound + (C + pairs) * U * f64(cost), deep, gap


def clearance(margin, p, q, pts, caps, obs, ocaps, d_p, d_q):
    """the whole unweighted cost of one goal (n,) in long double, its bound, the deepest penetration and the least gap: the point pairs from
    clearance_cases.clearance, the rest from capsule_pairs"""
    n = np.asarray(p).shape[0]
    pts64, obs64 = np.asarray(pts, dtype=np.float64).reshape(-1, 4), np.asarray(obs, dtype=np.float64).reshape(-1, 4)
    cost, bound, deep, gap = np.zeros(n, dtype=LD), np.zeros(n), np.zeros(n), np.full(n, np.inf)
    if pts64.shape[0] and obs64.shape[0]:
        cost, bound, deep = cc.clearance(margin, p, q, pts64, obs64, d_p, d_q)
        w = cc.world_points(p, q, pts64)
        o = np.asarray(obs64, dtype=LD)
        gap = np.asarray((np.sqrt(((w[:, :, None, :] - o[None, None, :, :3]) ** 2).sum(axis=3)) - np.asarray(pts64[:, 3], dtype=LD)[None, :, None] - o[None, None, :, 3]).min(axis=(1, 2)), dtype=np.float64)
    c2, b2, d2, g2 = capsule_pairs(margin, p, q, pts, caps, obs, ocaps, d_p, d_q)
    return cost + c2, bound + b2, np.maximum(deep, d2), np.minimum(gap, g2)


def goal_terms(t, tables, k, params, frames, dp, dq):
    """clearance(...) of goal k of the template (opcode 19 or 20) for frames {link: (p, q)} known to dp / dq {link: (n,)}"""
    g, off, m = t.goals[k], t.param_offsets[k], t.model
    n = next(iter(frames.values()))[0].shape[0]
    bc = lambda a: np.broadcast_to(a, (n,))  # noqa: E731
    link = m.link_index(g.link_name())
    if g.opcode == CLEAR:
        (p, q), d_p, d_q = frames[link], bc(dp[link]), bc(dq[link])
        return clearance(params[off], p, q, m.collision_points(link), m.collision_capsules(link), tables[k], np.zeros((0, 8)), d_p, d_q)
    other = m.link_index(g.getOtherLinkName())
    (pB, qB), (pA, qA) = frames[link], frames[other]
    p, q = bl.relative(pA, qA, pB, qB)
    d_p, d_q = bl.relative_bound(pA, qA, pB, qB, bc(dp[other]), bc(dq[other]), bc(dp[link]), bc(dq[link]))
    return clearance(params[off], p, q, m.collision_points(link), m.collision_capsules(link), m.collision_points(other), m.collision_capsules(other), d_p, d_q)


def costs_and_bounds(t, tables, params, frames, dp, dq, depth=None, gaps=None):
    """weighted cost (n, n_goals) in long double and its bound; the goals that are neither opcode 19 nor 20: tests/touch_cases.py.  `depth` / `gaps` (optional
    dicts): per clearance goal its deepest penetration and its least gap (n,)"""
    n = next(iter(frames.values()))[0].shape[0]
    cost = np.zeros((n, len(t.goals)), dtype=LD)
    bound = np.zeros((n, len(t.goals)))
    own = [k for k, g in enumerate(t.goals) if g.opcode in (CLEAR, SELF)]
    others = [k for k in range(len(t.goals)) if k not in own]
    if others:
        shim = types.SimpleNamespace(goals=[t.goals[k] for k in others], param_offsets=[t.param_offsets[k] for k in others], model=t.model)
        c, b = tc.costs_and_bounds(shim, None, params, frames, dp, dq)
        cost[:, others], bound[:, others] = c, b
    for k in own:
        c, b, deep, gap = goal_terms(t, tables, k, params, frames, dp, dq)
        w2 = LD(t.goals[k].getWeight()) ** 2
        cost[:, k] = c * w2
        bound[:, k] = float(w2) * b + C * U * np.abs(np.asarray(cost[:, k], dtype=np.float64))
        if depth is not None:
            depth[k] = deep
        if gaps is not None:
            gaps[k] = gap
    return cost, bound


# ---- models -------------------------------------------------------------------------------------------------------------------------------------------------
def capsules(k, seed, scale=0.08, rmin=0.0, rmax=0.05, lmin=0.05, lmax=0.25):
    """k rows ax ay az r bx by bz: first ends within `scale` of the link's origin, lengths lmin ... lmax in random directions"""
    rng = np.random.default_rng(9000 + seed)
    a = rng.uniform(-scale, scale, size=(k, 3))
    d = rng.normal(size=(k, 3))
    b = a + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(lmin, lmax, size=(k, 1))
    return np.hstack([a, rng.uniform(rmin, rmax, size=(k, 1)), b])


def with_shapes(model, link, n_points, n_capsules, seed, big=False):
    """`link` of `model` given n_points spheres and n_capsules capsules: small ones (a goal's link), or big ones (an other link: something penetrates)"""
    if n_points:
        model.add_collision_points(link, *(sc.balls(n_points, seed, 0.15, 0.35) if big else cc.spheres(n_points, seed)))
    if n_capsules:
        model.add_collision_capsules(link, capsules(n_capsules, seed, rmin=0.15, rmax=0.35) if big else capsules(n_capsules, seed))
    return model


def pad_model():
    m = pr2_like()
    m.add_link(PAD, RW, "r_pad_joint", "fixed", xyz=PAD_AT)
    return m


LINK_PRIMS = ((0, 1), (0, 2), (0, 3), (1, 1), (3, 2), (17, abi.MAX_LINK_CAPSULES))
OBSTACLES = (1, 2, 3, 9, abi.MAX_OBSTACLES)
SIDES = ((1, 0), (0, 1), (2, 1), (0, 3), (3, 2))
# geometry rows, placed deliberately.  Opcode 20 with the pad as the goal's link L and the wrist as the other link O: R is the translation PAD_AT for every
# individual (up to the rounding of the walk), so a row given in O's frame lies at (row - PAD_AT) in L's.  name -> (L points, L capsules, O points, O capsules,
# margin), everything in O's frame; the O capsule of most rows runs from (0, 0, 0.1) to (0.3, 0, 0.1) with radius 0.03.
_O = [[0.0, 0.0, 0.1, 0.03, 0.3, 0.0, 0.1]]
_TILT = 1e-9
GEOMETRY = {
    "sphere_beyond_first_end": ([[-0.05, 0.01, 0.1, 0.04]], [], [], _O, 0.01),                      # t clamps to 0
    "sphere_beyond_second_end": ([[0.36, -0.01, 0.1, 0.05]], [], [], _O, 0.01),                     # t clamps to 1
    "sphere_beside_the_middle": ([[0.15, 0.05, 0.1, 0.03]], [], [], _O, 0.01),
    "capsule_against_sphere_beyond_first_end": ([], _O, [[-0.05, 0.01, 0.1, 0.04]], [], 0.01),      # the same three with the capsule on L
    "capsule_against_sphere_beyond_second_end": ([], _O, [[0.36, -0.01, 0.1, 0.05]], [], 0.01),
    "capsule_against_sphere_beside_the_middle": ([], _O, [[0.15, 0.05, 0.1, 0.03]], [], 0.01),
    "parallel_overlapping": ([], [[0.1, 0.05, 0.1, 0.02, 0.4, 0.05, 0.1]], [], _O, 0.01),
    "parallel_offset_lengthwise": ([], [[0.32, 0.03, 0.1, 0.02, 0.6, 0.03, 0.1]], [], _O, 0.01),
    "crossing_at_right_angles": ([], [[0.15, -0.1, 0.14, 0.02, 0.15, 0.1, 0.14]], [], _O, 0.01),
    "end_to_end": ([], [[0.34, 0.0, 0.1, 0.02, 0.5, 0.0, 0.1]], [], _O, 0.01),
    "axes_1e-9_rad_apart": ([], [[0.05, 0.04, 0.1, 0.02, 0.35, 0.04 + 0.3 * _TILT, 0.1]], [], _O, 0.01),
    "negative_margin": ([[0.15, 0.05, 0.1, 0.03]], [[0.1, 0.05, 0.1, 0.02, 0.4, 0.05, 0.1]], [[0.2, 0.0, 0.1, 0.02]], _O, -1.0),  # every s <= 0: exactly 0
    "all_far": ([[50.0, 0.05, 0.1, 0.03]], [[50.1, 0.05, 0.1, 0.02, 50.4, 0.05, 0.1]], [[0.2, 0.0, 0.1, 0.02]], _O, 0.01),             # exactly 0
}
# a sphere beyond an end costs what a point sphere AT that end costs (within the two bounds): the twin model holds the end as a point row
END_TWINS = {"sphere_beyond_first_end": [[0.0, 0.0, 0.1, 0.03]], "sphere_beyond_second_end": [[0.3, 0.0, 0.1, 0.03]],
             "capsule_against_sphere_beyond_first_end": [[0.0, 0.0, 0.1, 0.03]], "capsule_against_sphere_beyond_second_end": [[0.3, 0.0, 0.1, 0.03]]}


def geometry_model(name, twin=False):
    lp, lc, op_, oc, _ = GEOMETRY[name]
    if twin:  # the capsule replaced by a point sphere at the end the sphere lies beyond
        if lc:
            lp, lc = END_TWINS[name], []
        else:
            op_, oc = END_TWINS[name], []
    m = pad_model()
    shift = np.array(PAD_AT)
    if len(lp):
        a = np.asarray(lp, dtype=np.float64)
        m.add_collision_points(PAD, a[:, :3] - shift, a[:, 3])
    if len(lc):
        a = np.asarray(lc, dtype=np.float64).copy()
        a[:, :3] -= shift
        a[:, 4:7] -= shift
        m.add_collision_capsules(PAD, a)
    if len(op_):
        a = np.asarray(op_, dtype=np.float64)
        m.add_collision_points(RW, a[:, :3], a[:, 3])
    if len(oc):
        m.add_collision_capsules(RW, oc)
    return m


@functools.lru_cache(maxsize=None)
def function_cases():
    """name -> (model, group, goals): the trip counts of every loop (zero trips of the point loops included), the caps, both states of the held-is-own bit, the
    places a based row can sit, the tables' places in the buffer, and the geometry rows"""
    out = {}
    for n, k in LINK_PRIMS:
        for m in OBSTACLES:
            out["c19_p%d_c%d_obstacles_%d" % (n, k, m)] = (with_shapes(pr2_like(), TIP, n, k, 3 * n + k), "right_arm", [ClearanceGoal(TIP, 0.01, cc.scene(m, 7 * n + m, rmin=0.15, rmax=0.35))])
    out["c19_p0_c1_obstacles_0"] = (with_shapes(pr2_like(), TIP, 0, 1, 1), "right_arm", [ClearanceGoal(TIP, 0.01)])  # the empty table: exactly 0
    for ln, lk in SIDES:
        for on, ok in SIDES:
            m = with_shapes(with_shapes(pr2_like(), RW, ln, lk, 10 * ln + lk), LW, on, ok, 10 * on + ok + 50, big=True)
            out["c20_L%d_%d_O%d_%d" % (ln, lk, on, ok)] = (m, "all", [SelfClearanceGoal(RW, LW, 0.01)])
    K = abi.MAX_LINK_CAPSULES
    out["c20_cap_L"] = (with_shapes(with_shapes(pr2_like(), RW, abi.MAX_TOUCH_POINTS - K, K, 71), LW, 0, 1, 72, big=True), "all", [SelfClearanceGoal(RW, LW, 0.01)])
    out["c20_cap_O"] = (with_shapes(with_shapes(pr2_like(), RW, 0, 1, 73), LW, abi.MAX_OBSTACLES - K, K, 74, big=True), "all", [SelfClearanceGoal(RW, LW, 0.01)])

    def pair(seed, link=RW, other=LW, model=None):
        return with_shapes(with_shapes(model or pr2_like(), link, 2, 1, seed), other, 1, 2, seed + 1, big=True)
    out["c20_other_first"] = (pair(80), "all", [PositionGoal(LW, (0.5, 0.2, 0.8)), SelfClearanceGoal(RW, LW, 0.01)])
    out["c20_other_last"] = (pair(82), "all", [PositionGoal(RW, (0.6, -0.2, 0.8)), SelfClearanceGoal(RW, LW, 0.01)])
    out["c20_elbow_against_wrist"] = (pair(84, RW, RE), "right_arm", [SelfClearanceGoal(RW, RE, 0.01)])
    out["c20_wrist_against_elbow"] = (pair(86, RE, RW), "right_arm", [SelfClearanceGoal(RE, RW, 0.01)])
    out["c20_other_is_root"] = (pair(88, RW, "base_link"), "right_arm", [SelfClearanceGoal(RW, "base_link", 0.01)])
    m = with_shapes(pair(90, LW, RW), RE, 4, 0, 91)  # (the TouchGoal's link: points only, tests/touch_cases.py restates it)
    u4 = (0.1, 0.2, 0.3, 0.9)
    out["c20_beside_pose_clearance_touch"] = (m, "all", [PoseGoal(RW, (0.6, -0.2, 0.8), u4), TouchGoal(RE, (0.55, -0.2, 0.7), (0.2, -0.3, 0.9), weight=0.7),
                                                         ClearanceGoal(LW, 0.01, cc.scene(9, 3, box=((0.2, -0.3, 0.4), (0.9, 0.7, 1.3))), weight=1.3), SelfClearanceGoal(LW, RW, 0.02, weight=0.6)])
    # a capsule of 0.45 m radius around the left wrist: a part of a random population's right wrists is inside (lanes that take the branch beside lanes that do not)
    m = with_shapes(pr2_like(), RW, 1, 1, 95)
    m.add_collision_capsules(LW, [[0.0, 0.0, -0.1, 0.45, 0.0, 0.0, 0.1]])
    out["c20_some_individuals"] = (m, "all", [SelfClearanceGoal(RW, LW, 0.0)])
    for name in GEOMETRY:
        out["geo_" + name] = (geometry_model(name), "right_arm", [SelfClearanceGoal(PAD, RW, GEOMETRY[name][4])])
    return out


def rows_of(name):
    """200 individuals; fewer where the restatement's (individuals x pairs) arrays would not fit (the counts stay: the loops run their full lengths on every row)"""
    return 16 if name.startswith("c19_p17_c64") else (48 if name.startswith("c20_cap") else 200)


# ---- function level -----------------------------------------------------------------------------------------------------------------------------------------
def exact_against(t, h, pr, seed, params, genes, stats, name):
    b = rr.Bounds(pr, pr.full(seed, genes).astype(np.float64))
    fr = tc.exact_frames(pr, seed, genes)
    gaps = {}
    cost, bound = costs_and_bounds(t, t.obstacle_tables(), params, fr, {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, gaps=gaps)
    pa, sa = h.fitness(abi.FK_EXACT, seed, params, genes)
    want, bnd = tc.sums(t, cost, bound)[0]
    err = np.abs(pa - want)
    r = stats.ratio("exact primary", err, np.maximum(bnd, 1e-300), name)
    worst = int(np.argmax(err / np.maximum(bnd, 1e-300)))
    assert np.all(np.isfinite(pa)), name
    assert r <= 1.0, "%s: exact primary fitness off by %.3g, bound %.3g (row %d)" % (name, err.max(), bnd[worst], worst)
    assert not sa.any(), name
    return pa, cost, bnd, b, fr, gaps


def function_level(make_solver, name, stats):
    """bioik_eval_fitness in both FK modes and bioik_eval_check against the restatement; the worst error / bound ratios go to `stats`.  Returns the fitness arrays."""
    model, group, goals = function_cases()[name]
    n = rows_of(name)
    t, h, pr, seed, genes = sc.setup(make_solver, model, group, goals, name, n)
    params = t.pack_params()
    pa, cost, bnd, b, fr, gaps = exact_against(t, h, pr, seed, params, genes, stats, name)
    own = [k for k, g in enumerate(t.goals) if g.opcode in (CLEAR, SELF)]
    if name.endswith("obstacles_0") or name in ("geo_negative_margin", "geo_all_far"):
        assert np.all(pa == 0.0) and np.all(np.asarray(cost[:, own], dtype=np.float64) == 0.0), name  # exactly nothing, not "small"
    elif name.startswith("geo_"):
        assert np.all(pa > 0.0), name  # (placed to penetrate)
    elif name.startswith(("c19_p", "c20_L", "c20_cap")):
        assert np.any(pa > 0.0), name  # (every case of the grids takes the branch somewhere)
    if name == "c20_some_individuals":
        for hit in (int(np.count_nonzero(np.asarray(cost[:, 0], dtype=np.float64) > 0.0)), int(np.count_nonzero(pa > 0.0))):
            assert n // 20 < hit < n - n // 20, (name, hit)
    if name[4:] in END_TWINS:  # the same sphere against a point sphere at the end it lies beyond
        t2, h2, pr2, seed2, genes2 = sc.setup(make_solver, geometry_model(name[4:], twin=True), group, goals, name, n)
        pb, _, bnd2, _, _, _ = exact_against(t2, h2, pr2, seed2, params, genes2, rr.Stats(), name + " (twin)")
        h2.close()
        assert np.all(np.abs(pa - pb) <= bnd + bnd2), (name, np.abs(pa - pb).max())
    # the success test (the default branch): weighted cost < min(dpos, dtwist)^2.  Per row the margin of every clearance goal is set from the row's own least gap:
    # 1 mm below it nothing penetrates, provably a success; 1 cm / weight above it some pair penetrates by that much, provably none (clearance_cases.function_level)
    if len(own) == len(t.goals) and not name.endswith("obstacles_0"):
        sp = abi.default_solve_params(dpos=-1.0, drot=-1.0, dtwist=1e-3)
        rows = list(range(0, n, max(n // 8, 1)))
        hits = 0
        for j, i in enumerate(rows):
            P1 = params.copy()
            for k in own:
                P1[t.param_offsets[k]] = gaps[k][i] + (-1e-3 if j % 2 == 0 else 1e-2 / abs(t.goals[k].getWeight()))
            f1 = {l: (fr[l][0][i:i + 1], fr[l][1][i:i + 1]) for l in fr}
            c1, b1 = costs_and_bounds(t, t.obstacle_tables(), P1, f1, {l: b.dp(l)[i:i + 1] for l in b.m}, {l: b.dq(l)[i:i + 1] for l in b.m})
            ok = int(h.check(sp, seed, P1, genes[i:i + 1])[0])
            sure_yes = all(float(c1[0, k]) + b1[0, k] < 1e-6 for k in own)
            sure_no = any(float(c1[0, k]) - b1[0, k] >= 1e-6 for k in own)
            assert sure_yes == (j % 2 == 0) and sure_no == (j % 2 == 1), (name, i, [float(c1[0, k]) for k in own])
            assert ok == (1 if sure_yes else 0), (name, i, ok, [float(c1[0, k]) for k in own])
            hits += ok
        assert hits == (len(rows) + 1) // 2, (name, hits)
    # linearised phenotypes around a base: the frames from the unnormalised quaternions as they are
    rng = np.random.default_rng(len(name))
    base = genes[0]
    near = np.ascontiguousarray(base + 0.02 * rng.normal(size=(max(n // 8, 4), len(pr.active))))
    tb_l, dl_l = pr.approximator(seed, base)
    dpl, dql = sc.linear_bounds(pr, seed, base, near, dl_l)
    cost, bound = costs_and_bounds(t, t.obstacle_tables(), params, pr.linear_frames(tb_l, dl_l, base, near), dpl, dql)
    pl, _ = h.fitness(abi.FK_LINEAR, seed, params, near, base)
    want, bnd = tc.sums(t, cost, bound)[0]
    err = np.abs(pl - want)
    r = stats.ratio("linear primary", err, np.maximum(bnd, 1e-300), name)
    assert np.all(np.isfinite(pl)), name
    assert r <= 1.0, "%s: linearised primary fitness off by %.3g, bound %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))])
    h.close()
    return pa, pl


def symmetry(make_solver, stats, n=200):
    """goal (L, O) and goal (O, L) state the same distances: under exact FK they agree within the sum of their bounds"""
    model = with_shapes(with_shapes(pr2_like(), RW, 2, 2, 31, big=True), LW, 1, 3, 32, big=True)
    res = []
    for goal in (SelfClearanceGoal(RW, LW, 0.01), SelfClearanceGoal(LW, RW, 0.01)):
        t, h, pr, seed, genes = sc.setup(make_solver, model, "all", [goal], "symmetry", n)
        pa, _, bnd, _, _, _ = exact_against(t, h, pr, seed, t.pack_params(), genes, stats, "symmetry")
        res.append((pa, bnd))
        h.close()
    (a, ba), (b, bb) = res
    assert np.any(a > 0.0) and np.all(np.abs(a - b) <= ba + bb), np.abs(a - b).max()


def zero_quaternion(make_solver):
    """a finite input never yields a NaN or an infinity: bioik_eval_fitness over linearised phenotypes FAR from their base (the extrapolated quaternions are nowhere
    near unit length and the segments stretch or shrink), finite on every row"""
    for name in ("c19_p1_c1_obstacles_3", "c20_L2_1_O3_2"):
        model, group, goals = function_cases()[name]
        t, h, pr, seed, genes = sc.setup(make_solver, model, group, goals, name, 64)
        far = np.ascontiguousarray(genes[0] + np.linspace(-40.0, 40.0, 64)[:, None] * np.ones(len(pr.active)))
        pl, _ = h.fitness(abi.FK_LINEAR, seed, t.pack_params(), far, genes[0])
        assert np.all(np.isfinite(pl)), name
        h.close()


def touch_twins(make_solver, n=200):
    """TouchGoal on a link with one box and one capsule: both FK modes bit for bit the same model with the capsule's two end spheres as point rows"""
    cap = [0.02, -0.01, 0.03, 0.025, 0.12, 0.04, -0.05]
    a, b = pr2_like(), pr2_like()
    for m in (a, b):
        m.add_collision_box(TIP, tc.BOX)
    a.add_collision_capsules(TIP, [cap])
    b.add_collision_points(TIP, [cap[:3], cap[4:7]], [cap[3], cap[3]])
    goal = [TouchGoal(TIP, (0.55, -0.2, 0.7), (0.2, -0.3, 0.9))]
    res = []
    for m in (a, b):
        t, h, pr, seed, genes = sc.setup(make_solver, m, "right_arm", goal, "touch_twins", n)
        near = np.ascontiguousarray(genes[0] + 0.02 * np.random.default_rng(1).normal(size=(25, len(pr.active))))
        res.append((h.fitness(abi.FK_EXACT, seed, t.pack_params(), genes)[0], h.fitness(abi.FK_LINEAR, seed, t.pack_params(), near, genes[0])[0]))
        h.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.ptp(res[0][0]) > 0.0
    only = pr2_like()  # a link that carries nothing but a capsule is accepted too
    only.add_collision_capsules(TIP, [cap])
    make_solver(ProblemTemplate(only, "right_arm", goal)).close()
    return res[0]


def unchanged_bits(make_solver):
    """a model without capsules gives exactly the bits it gave before links could carry capsules (tools/record_clearance_bits.py, recorded on that commit)"""
    want = np.load(GOLDEN)
    got = record_clearance_bits.bits(make_solver)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------------------------
N_QUERIES, SOLVE, DTWIST, MARGIN, VARIANTS = sc.N_QUERIES, dict(cc.SOLVE), 1e-5, 0.01, sc.VARIANTS
FOREARM_CAPSULE = [0.05, 0.0, 0.0, 0.08, 0.25, 0.0, 0.0]  # the hull of self_clearance_cases.FOREARM_SPHERES
TARGET_SEED = 13


def solve_model():
    m = pr2_like()
    for l in (RF, LF):
        m.add_collision_capsules(l, [FOREARM_CAPSULE])
    return m


def solve_template(goals=True):
    return ProblemTemplate(solve_model(), "all", [PositionGoal(RW), PositionGoal(LW)] + ([SelfClearanceGoal(RF, LF, MARGIN)] if goals else []))


def forearm_depth(m, x, margin=0.0):
    """how deep the forearm capsules are inside one another at the full variable vectors x (n, V): long double on the float64 frames of bio_ik_amd.robot"""
    out = np.zeros(len(x))
    z = np.zeros(1)
    for i, xi in enumerate(x):
        a, b = (np.asarray(link_transform(m, m.link_index(l), xi)) for l in (LF, RF))
        p, q = bl.relative(a[None, :3], a[None, 3:], b[None, :3], b[None, 3:])
        out[i] = capsule_pairs(margin, p, q, np.zeros((0, 4)), m.collision_capsules(RF), np.zeros((0, 4)), m.collision_capsules(LF), z, z)[2][0]
    return out


@functools.lru_cache(maxsize=None)
def targets_and_seeds(n, seed):
    """self_clearance_cases.targets_and_seeds with the CAPSULES clear by twice the margin at the target configuration, so that an answer exists"""
    m = solve_model()
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    torso = m.variable_index("torso_lift_joint")
    targets, seeds = [], []
    while len(targets) < n:
        x = lo + (hi - lo) * rng.random(m.n_variables)
        x[torso] = 0.1
        r, l = (np.asarray(link_transform(m, m.link_index(k), x))[:3] for k in (RW, LW))
        if not (r[0] > 0.35 and l[0] > 0.35 and r[1] - l[1] > sc.CROSS and abs(r[2] - l[2]) < 0.25):
            continue
        if forearm_depth(m, x[None], 2 * MARGIN)[0] > 0.0:
            continue
        s = lo + (hi - lo) * rng.random(m.n_variables)
        s[torso] = 0.1
        targets.append(np.concatenate([r, l]))
        seeds.append(s)
    targets, seeds = np.ascontiguousarray(targets), np.ascontiguousarray(seeds)
    targets.setflags(write=False), seeds.setflags(write=False)
    return targets, seeds


def queries(t, n=N_QUERIES, seed=TARGET_SEED):
    targets, seeds = targets_and_seeds(n, seed)
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        params[:, off:off + len(g.params())] = g.params()[None]
    params[:, 0:3], params[:, 3:6] = targets[:, :3], targets[:, 3:]
    return seeds.copy(), params


def verify_solve(t, h, seeds, params, sol, fit, suc):
    """on the returned joint values, recomputed in long double: every row flagged a success has no pair deeper than dtwist / weight up to the bound of the cost, and
    its PositionGoals within 3 dtwist^2; the fitness is the long-double cost within its bound.  Returns per row the deepest penetration at the goals' margins."""
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    inactive = np.setdiff1d(np.arange(h.V), pr.active)
    deepest = np.zeros(sol.shape[0])
    for i in range(sol.shape[0]):
        b = rr.Bounds(pr, sol[i:i + 1].astype(np.float64))
        depth = {}
        cost, bound = costs_and_bounds(t, t.obstacle_tables(), params[i], tc.exact_frames(pr, sol[i], sol[i:i + 1, pr.active]), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, depth)
        assert np.array_equal(sol[i, inactive], seeds[i, inactive])
        if suc[i]:
            for k, g in enumerate(t.goals):
                limit = (3 if g.opcode == abi.GOAL_POSITION else (2 if g.opcode == abi.GOAL_POSE else 1)) * DTWIST ** 2
                assert float(cost[0, k]) < limit + bound[0, k], (i, k, float(cost[0, k]), bound[0, k])
                if k in depth:
                    assert (depth[k][0] * g.getWeight()) ** 2 < DTWIST ** 2 + bound[0, k], (i, k, depth[k][0])
        want = float(cost[0].sum())
        assert abs(fit[i] - want) <= bound[0].sum() + C * U * want, (i, fit[i], want)
        deepest[i] = max([depth[k][0] for k in depth] + [0.0])
    return deepest


STEERING = {}
# found on the host simulator (= the device, bit for bit) and asserted as found: WITHOUT the SelfClearanceGoal this many of the 16 answers have forearm capsules more
# than 1 cm inside one another; WITH it this many of the 16 succeed
WITHOUT_PENETRATING, WITH_SUCCESS = 7, 16


def whole_solve(make_solver, variant="primary"):
    """Returns (solver, template, seeds, params, solve parameters, results) for bit comparisons."""
    t = solve_template()
    h = make_solver(t)
    seeds, params = queries(t)
    p, res = sc.run(h, t, variant, seeds, params)
    if variant == "bounded":
        seeds, (lo, hi) = sc.solve_bounds(t, seeds)
        assert np.all(res[0] >= lo) and np.all(res[0] <= hi)
    if variant == "ranked":
        sol, fit, suc, steps, count = res
        assert count.min() >= 1
        for r in range(2):
            rows = count > r
            verify_solve(t, h, seeds[rows], params[rows], sol[rows, r], fit[rows, r], suc[rows, r])
    else:
        verify_solve(t, h, seeds, params, res[0], res[1], res[2])
    if variant == "primary":
        steering(make_solver, seeds, p, res)
    return h, t, seeds, params, p, res


def steering(make_solver, seeds, p, with_goals):
    t0 = solve_template(goals=False)
    h0 = make_solver(t0)
    _, params0 = queries(t0)
    sol0, _, suc0, _ = h0.solve_batch(p, seeds, params0)
    h0.close()
    sol1, _, suc1, _ = with_goals
    deep0, deep1 = forearm_depth(t0.model, sol0), forearm_depth(t0.model, sol1)
    STEERING.update(without_penetrating=int(np.count_nonzero(deep0 > 0.01)), without_success=int(suc0.sum()), with_success=int(suc1.sum()),
                    with_penetrating=int(np.count_nonzero(deep1 > 0.01)))
    assert STEERING["without_penetrating"] == WITHOUT_PENETRATING >= 4, (STEERING, deep0)
    assert STEERING["with_success"] == WITH_SUCCESS == N_QUERIES, (STEERING, suc1)
    assert np.all(deep1[suc1 != 0] == 0.0)  # (clear by the margin up to dtwist: at margin 0 nothing touches)


# ---- the second solve, opcode 19: the right arm with a capsule on its forearm behind clearance_cases' column of nine spheres ---------------------------------------
ARM_STEERING = {}
ARM_TARGET_SEED = 11
# found on the host simulator and asserted as found: answers more than 1 cm inside the column WITHOUT the goal; successes WITH it
ARM_WITHOUT_PENETRATING, ARM_WITH_SUCCESS = 5, 16
ARM_CAPSULE = [0.05, 0.0, 0.0, 0.05, 0.25, 0.0, 0.0]  # the hull of clearance_cases.solve_model's three forearm spheres


def arm_model():
    m = pr2_like()
    m.add_collision_capsules(cc.FOREARM, [ARM_CAPSULE])
    return m


def arm_template(goals=True):
    return ProblemTemplate(arm_model(), "right_arm", [PositionGoal(TIP)] + ([ClearanceGoal(cc.FOREARM, cc.MARGIN, cc.COLUMN)] if goals else []))


def arm_depth(m, x, margin=0.0):
    """how deep the forearm capsule is inside the column at the full variable vectors x (n, V)"""
    out = np.zeros(len(x))
    z = np.zeros(1)
    for i, xi in enumerate(x):
        f = np.asarray(link_transform(m, m.link_index(cc.FOREARM), xi))
        out[i] = capsule_pairs(margin, f[None, :3], f[None, 3:], np.zeros((0, 4)), m.collision_capsules(cc.FOREARM), cc.COLUMN, np.zeros((0, 8)), z, z)[2][0]
    return out


@functools.lru_cache(maxsize=None)
def arm_targets_and_seeds(n, seed):
    """clearance_cases.targets_and_seeds with the CAPSULE clear of the column by twice the margin at the target configuration"""
    m = arm_model()
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    torso = m.variable_index("torso_lift_joint")
    targets, seeds = [], []
    while len(targets) < n:
        x = lo + (hi - lo) * rng.random(m.n_variables)
        x[torso] = 0.1
        tip = np.asarray(link_transform(m, m.link_index(TIP), x))
        if not (tip[0] > 0.55 and -0.5 < tip[1] < 0.0) or arm_depth(m, x[None], 2 * cc.MARGIN)[0] > 0.0:
            continue
        s = lo + (hi - lo) * rng.random(m.n_variables)
        s[torso] = 0.1
        targets.append(tip[:3])
        seeds.append(s)
    targets, seeds = np.ascontiguousarray(targets), np.ascontiguousarray(seeds)
    targets.setflags(write=False), seeds.setflags(write=False)
    return targets, seeds


def arm_queries(t, n=N_QUERIES, seed=ARM_TARGET_SEED):
    targets, seeds = arm_targets_and_seeds(n, seed)
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        params[:, off:off + len(g.params())] = g.params()[None]
    params[:, 0:3] = targets
    return seeds.copy(), params


def arm_solve(make_solver):
    """Returns (solver, template, seeds, params, solve parameters, results); asserts verify_solve and the two conditions"""
    t, t0 = arm_template(), arm_template(goals=False)
    h, h0 = make_solver(t), make_solver(t0)
    seeds, params = arm_queries(t)
    p = abi.default_solve_params(**SOLVE)
    res = h.solve_batch(p, seeds, params)
    verify_solve(t, h, seeds, params, res[0], res[1], res[2])
    sol0, _, suc0, _ = h0.solve_batch(p, seeds, arm_queries(t0)[1])
    h0.close()
    deep0, deep1 = arm_depth(t.model, sol0), arm_depth(t.model, res[0])
    ARM_STEERING.update(without_penetrating=int(np.count_nonzero(deep0 > 0.01)), without_success=int(suc0.sum()), with_success=int(res[2].sum()),
                        with_penetrating=int(np.count_nonzero(deep1 > 0.01)))
    assert ARM_STEERING["without_penetrating"] == ARM_WITHOUT_PENETRATING >= 4, (ARM_STEERING, deep0)
    assert ARM_STEERING["with_success"] == ARM_WITH_SUCCESS == N_QUERIES, (ARM_STEERING, res[2])
    assert np.all(deep1[res[2] != 0] == 0.0)
    return h, t, seeds, params, p, res


def mapping_independence(make_solver, monkeypatch, **kw):
    """self_clearance_cases.mapping_independence, as it stands, on the capsule problem"""
    monkeypatch.setattr(sc, "solve_template", solve_template)
    monkeypatch.setattr(sc, "queries", queries)
    sc.mapping_independence(make_solver, monkeypatch, **kw)
