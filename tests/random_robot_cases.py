"""Random robots and goal lists (tools/robot_gen.py) on the library under test: the GPU suite (tests/test_gpu_random_robots.py, libbioik_hip.so on the device)
and the host simulator (tests/test_hostsim_random_robots.py, the same kernel bodies built for the host).  Three levels per case:

  (a) function level against long double (tests/np_fk.py, tests/np_goals.py), under the default (folded) joint program and under BIOIK_COMPILE_EXACT=1:
      eval_fk, eval_fitness (exact and linearised), eval_approximator and eval_check, on random configurations and on edge inputs, each against an error
      bound derived from the model stated in `Bounds`;
  (b) whole solves bit for bit against the oracle on goal lists in walk order, spread over modes, populations, islands and the launcher's kernels;
  (c) the result contract of solves that cannot be bit-compared with anything (default program, goals in any order);
  (d) joint angles from 1e5 rad to the end of the shared sincos's domain (BIOIK_SINCOS_DOMAIN, read from the library under test) on three small robots: FK, fitness and
      the success test against long double WITHOUT the `Theta` term of the bounds, FK bit for bit against the oracle under the exact program.

`make_solver(template)` makes a bioik_amd.solver.HipSolver of the library under test; `report` is a limit_cases.Report (BIOIK_SOLVE_REPORT through capfd)."""
import contextlib
import os

import numpy as np

import np_goals
from bio_ik_amd import abi, solver
from bio_ik_amd.workload import make_queries
from np_fk import LD, quat_from_rot_batch
from oracle import orc
from tools import robot_gen

U = 2.0 ** -53
C = 64  # one constant for every bound of this file (see Bounds), at most 64: a few roundings per link
DBL_MAX = np.finfo(np.float64).max

# the fixed seed set: every seed a case of random_case (seeds whose tree has no moving joint are skipped by the generator)
SEEDS = list(range(1, 41))
# ... for the result contract: seeds whose goal lists the solver meets now and then with secondary goals present (8, 26, 39), and others
CONTRACT_SEEDS = sorted(set(SEEDS[1::3]) | {8, 26, 39})
KERNELS = ("k_solve", "k_solve_lean", "k_solve_lean_cl", "k_solve_lean_cl4", "k_solve_lean_cl4h", "k_solve_lean_cl64w4", "k_solve_lean_lin",
           "k_solve_lean_clj4", "k_solve_point")


def cases(seeds=SEEDS, **kw):
    return [c for c in (robot_gen.random_case(s, **kw) for s in seeds) if c is not None]


@contextlib.contextmanager
def program(exact):
    """BIOIK_COMPILE_EXACT for the handles made inside the block"""
    prev = os.environ.get("BIOIK_COMPILE_EXACT")
    os.environ["BIOIK_COMPILE_EXACT"] = "1" if exact else "0"
    try:
        yield
    finally:
        if prev is None:
            del os.environ["BIOIK_COMPILE_EXACT"]
        else:
            os.environ["BIOIK_COMPILE_EXACT"] = prev


def solve_params(**kw):
    return abi.default_solve_params(**kw)


def thresholds(p):
    """dpos, drot, dtwist as the reference takes them (a negative value: not tested, DBL_MAX)"""
    return tuple(DBL_MAX if v < 0 else float(v) for v in (p.dpos, p.drot, p.dtwist))


class Stats:
    """the worst measured error / bound ratio per quantity, and the near-threshold success cases"""

    def __init__(self):
        self.worst = {}
        self.band = 0
        self.rows = 0

    def ratio(self, what, err, bound, where=""):
        r = float(np.max(np.asarray(err, dtype=np.float64) / np.maximum(np.asarray(bound, dtype=np.float64), 1e-300))) if np.size(err) else 0.0
        if r > self.worst.get(what, (0.0, ""))[0]:
            self.worst[what] = (r, where)
        return r

    def line(self):
        return "worst error / bound (C = %d): " % C + ", ".join("%s %.3g" % (k, v[0]) for k, v in sorted(self.worst.items())) + \
            " | success decisions inside the band: %d of %d" % (self.band, self.rows)


class Bounds:
    """The error model.  u = 2^-53; C is fixed for the whole file.

    FK of a tip with m links on its chain: every link composes one constant frame and one joint frame, each a few roundings in the rotation and in the
    translation; a sincos of a continuous joint at |theta| adds the rounding of its argument reduction, u |theta|.  So
        |dp| <= C u (m + 1 + Theta) Lambda,   min over +-q of |dq| <= C u (m + 1 + Theta),
    Lambda = 1 + sum over the chain of |origin offset| + |prismatic displacement| + |floating / planar translation|, Theta = sum of |theta| / pi over the
    chain's revolute joints (at most a few units for angles in [-pi, pi]; up to 1e5 at the edge draw).
    Costs: a squared residual r whose vector is known to dr costs 2 |r| dr + dr^2, plus C u of the cost for its own arithmetic.  The residual of each goal
    moves with dp and dq as its expression says (np_goals.link_cost): a rotated unit vector by 2 dq, a normalised difference by dp / its length; Cone's
    angle acos(x) by dx / sqrt(1 - x^2), and by no more than sqrt(2 dx) where 1 - x^2 is below dx (acos is 1/2-Hoelder at +-1).
    Approximator columns of revolute / prismatic genes: the products of frames already bounded, |dcol| <= C u (m + 1 + Theta) (Lambda + 1) |sum of factors|.
    Floating / planar columns: a forward difference over h = 1e-5 of two frames, each off by the FK bound -- amplified by 1 / h -- and a rotation angle
    2 acos(w) near w = 1, which is 1/2-Hoelder: |dcol| <= (C u (m + 1) (Lambda + 1) + 4 sqrt(2 C u (m + 1))) / h.
    Linearised frames: tip + sum delta_k dv_k, so |df| <= |dtip| + sum |ddelta_k| |dv_k| + C u sum |delta_k| |dv_k|.
    Success: a decision may differ only where a tested quantity lies within its bound of the threshold: a distance by dp, an angle (degrees) by
    180 / pi * 2 dx / max(sqrt(1 - x^2), sqrt(dx)) with dx = 2 dq, a twist component by dp + 2 dq |Delta p| (linear) or 4 dq (angular), a cost by its bound."""

    def __init__(self, pr, X):
        """pr: np_goals.Problem; X: (n, V) full variable vectors"""
        m = pr.model
        self.pr = pr
        n = X.shape[0]
        self.m, self.lam, self.theta = {}, {}, {}
        for t in set(pr.tips) | set(int(l) for l in np.nonzero(np.asarray(m.link_mass) > 0)[0]):
            chain = robot_gen.chain_of(m, t)
            lam = np.ones(n)
            th = np.zeros(n)
            for l in chain:
                lam += np.linalg.norm(np.asarray(m.link_origin[l][:3]))
                jt, fv = m.joint_type[l], m.joint_first_variable[l]
                src = fv
                if m.joint_mimic[l] >= 0:  # (the follower's value is the leader's times its factor)
                    k, f = l, 1.0
                    while m.joint_mimic[k] >= 0:
                        f, k = f * abs(m.joint_mimic_factor[k]), m.joint_mimic[k]
                    src = m.joint_first_variable[k]
                else:
                    f = 1.0
                if jt == abi.JOINT_PRISMATIC:
                    lam += f * np.abs(X[:, src]) + abs(m.joint_mimic_offset[l])
                elif jt == abi.JOINT_REVOLUTE:
                    th += (f * np.abs(X[:, src]) + abs(m.joint_mimic_offset[l])) / np.pi
                elif jt == abi.JOINT_FLOATING:
                    lam += np.linalg.norm(X[:, fv:fv + 3], axis=1)
                elif jt == abi.JOINT_PLANAR:
                    lam += np.linalg.norm(X[:, fv:fv + 2], axis=1)
                    th += np.abs(X[:, fv + 2]) / np.pi
            self.m[t], self.lam[t], self.theta[t] = len(chain), lam, th

    def dq(self, t):
        return C * U * (self.m[t] + 1 + self.theta[t])

    def dp(self, t):
        return self.dq(t) * self.lam[t]


def sq_bound(r, dr):
    return 2 * np.abs(r) * dr + dr * dr


def joint_set_bound(pr, op, P, genes, seed, goal):
    """the goals over the joint values: each term's residual is a difference of two doubles that are themselves rounded (the limits' midpoint, the
    displacement factors), so it is known to C u (|gene| + |other| + span) times its factor; squared residuals as above"""
    g = np.asarray(genes, dtype=np.float64)
    s = np.asarray(seed, dtype=np.float64)
    mid, span, w, bd = (np.asarray(a, dtype=np.float64) for a in (pr.mid, pr.span, pr.w, pr.bounded))
    if op in (abi.GOAL_AVOID_JOINT_LIMITS, abi.GOAL_CENTER_JOINTS):
        r = (np.abs(g - mid) * 2 + span) * w * bd
        dr = C * U * (np.abs(g) + np.abs(mid) + span) * 2 * w * bd
        return np.sum(sq_bound(r, dr), axis=1)
    if op in (abi.GOAL_REGULARIZATION, abi.GOAL_MINIMAL_DISPLACEMENT):
        r = np.abs(g - s[pr.active]) * (w if op == abi.GOAL_MINIMAL_DISPLACEMENT else 1.0)
        return np.sum(sq_bound(r, C * U * r), axis=1)
    v = pr.model.variable_index(goal.variable_name())
    where = np.nonzero(pr.active == v)[0]
    x = g[:, where[0]] if len(where) else np.full(g.shape[0], s[v])
    return sq_bound(np.abs(P[0] - x), C * U * (abs(P[0]) + np.abs(x)))


def cost_bounds(pr, params, p, q, dp, dq, genes_cost, genes=None, seed=None):
    """per goal (n, n_goals) bounds on the weighted cost, for frames p / q of the tips known to dp / dq ({link: (n,)}), costs genes_cost (n, n_goals)"""
    n = genes_cost.shape[0]
    out = np.zeros((n, len(pr.template.goals)))
    for k, (goal, off) in enumerate(zip(pr.template.goals, pr.template.param_offsets)):
        op = goal.opcode
        P = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[op]], dtype=np.float64)
        w2 = goal.getWeight() ** 2
        own = C * U * np.abs(np.asarray(genes_cost[:, k], dtype=np.float64))
        if op in np_goals.JOINT_SET:
            out[:, k] = w2 * joint_set_bound(pr, op, P, genes, seed, goal) + own
            continue
        if op == abi.GOAL_BALANCE:
            m = pr.model
            mass = np.asarray(m.link_mass)
            db = sum(mass[l] / mass.sum() * (dp[int(l)] + 2 * dq[int(l)] * np.linalg.norm(m.link_center[l])) for l in np.nonzero(mass > 0)[0])
            r = np.sqrt(np.asarray(genes_cost[:, k], dtype=np.float64) / w2)
            out[:, k] = w2 * sq_bound(r, 2 * db) + own
            continue
        link = pr.model.link_index(goal.link_name())
        pl, ql = np.asarray(p[link], dtype=np.float64), np.asarray(q[link], dtype=np.float64)
        d_p, d_q = dp[link], dq[link]
        qn = np.linalg.norm(ql, axis=1)
        rot = 2 * d_q * (1 + qn * qn)  # (a vector rotated by a quaternion known to dq: 2 dq per unit length, the norm of an unnormalised q squared)
        if op == abi.GOAL_POSITION:
            b = sq_bound(np.linalg.norm(pl - P[:3], axis=1), d_p)
        elif op == abi.GOAL_ORIENTATION:
            b = sq_bound(np.minimum(np.linalg.norm(P[:4] - ql, axis=1), np.linalg.norm(P[:4] + ql, axis=1)), d_q)
        elif op == abi.GOAL_POSE:
            b = sq_bound(np.linalg.norm(pl - P[:3], axis=1), d_p) + P[7] ** 2 * sq_bound(
                np.minimum(np.linalg.norm(P[3:7] - ql, axis=1), np.linalg.norm(P[3:7] + ql, axis=1)), d_q)
        elif op == abi.GOAL_LOOK_AT:
            dist = np.linalg.norm(P[3:6] - pl, axis=1)
            b = sq_bound(2.0, d_p / np.maximum(dist, 1e-300) * 2 + rot * 2)
        elif op in (abi.GOAL_MAX_DISTANCE, abi.GOAL_MIN_DISTANCE):
            d = np.linalg.norm(pl - P[:3], axis=1)
            b = sq_bound(np.abs(d - P[3]), d_p)
        elif op == abi.GOAL_LINE:
            r = P[:3] - (pl - P[None, 3:6] * ((pl - P[:3]) @ P[3:6])[:, None])
            b = sq_bound(np.linalg.norm(r, axis=1), d_p * (1 + P[3:6] @ P[3:6]))
        elif op == abi.GOAL_PLANE:
            b = sq_bound(np.abs((pl - P[:3]) @ P[3:6]), d_p * np.linalg.norm(P[3:6]))
        elif op == abi.GOAL_SIDE:
            b = sq_bound(np.linalg.norm(P[:3]) * np.linalg.norm(P[3:6]) * (1 + qn * qn), rot * np.linalg.norm(P[:3]) * np.linalg.norm(P[3:6]))
        elif op == abi.GOAL_DIRECTION:
            b = sq_bound(np.linalg.norm(P[:3]) * (1 + qn * qn) + np.linalg.norm(P[3:6]), rot * np.linalg.norm(P[:3]))
        elif op == abi.GOAL_CONE:
            v = np.asarray(np_goals.qrot(np.asarray(ql, dtype=LD), P[4:7]), dtype=np.float64)
            x = np.clip((v @ P[7:10]) / np.sqrt(np.sum(v * v, axis=1) * (P[7:10] @ P[7:10])), -1, 1)
            dx = rot + C * U
            dang = np.minimum(dx / np.maximum(np.sqrt(np.maximum(1 - x * x, 0)), 1e-300), np.sqrt(2 * dx))
            ang = np.arccos(x)
            b = sq_bound(np.maximum(0, ang - P[10]), dang) + P[3] ** 2 * sq_bound(np.linalg.norm(P[:3] - pl, axis=1), d_p)
        else:
            raise AssertionError(op)
        out[:, k] = w2 * b + own
    return out


def tip_index(h):
    return {int(l): i for i, l in enumerate(h.tip_links)}


def device_frames(h, seed, genes):
    """{link: (p, q)} of the device's exact FK"""
    f = h.fk_genes(seed, genes)
    return {int(l): (f[:, i, :3], f[:, i, 3:]) for i, l in enumerate(h.tip_links)}


def edge_configurations(case, pr, rng, n):
    """configurations at the edges of the joints' ranges: continuous joints at multiples of pi / 2 and at |theta| up to 1e5, prismatic joints (and the
    bounded translations) at full extension, floating joints at quaternions of norm 0.5 ... 2"""
    m = case.model
    X = robot_gen.sample_configurations(m, rng, n)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    for v in range(m.n_variables):
        name = m.variable_names[v]
        if not m.var_bounded[v] and "/" not in name:  # continuous
            X[:, v] = np.where(rng.random(n) < 0.5, rng.integers(-8, 9, size=n) * (np.pi / 2), rng.choice([-1, 1], size=n) * 10.0 ** rng.uniform(0, 5, size=n))
        elif m.var_bounded[v] and not name.split("/")[-1].startswith("rot_"):
            X[:, v] = np.where(rng.random(n) < 0.6, np.where(rng.random(n) < 0.5, lo[v], hi[v]), X[:, v])
    return X


def edge_params(case, pr, params, seed, genes, rng):
    """goal parameters that put every link goal of the case on an edge for ONE configuration (frames of long-double FK): goals met exactly, q against -q,
    180 degree rotation errors, Cone at its bound +- a few ulps, LookAt targets almost on the axis, Min/MaxDistance at distance = r +- tiny, points on the
    Line or Plane, Side with a dot product of 0"""
    R, p = pr.frames(seed, genes[None])
    P = np.array(params, dtype=np.float64)
    for goal, off in zip(case.goals, pr.template.param_offsets):
        if goal.link_name() is None:
            continue
        l = pr.model.link_index(goal.link_name())
        pl = np.asarray(p[l, 0], dtype=np.float64)
        Rl = R[l, 0]
        ql = np.asarray(quat_from_rot_batch(R[l])[0], dtype=np.float64)
        op = goal.opcode
        k = int(rng.integers(3))
        tiny = float(rng.choice([0.0, 1e-15, -1e-15, 1e-12, -1e-12]))
        if op == abi.GOAL_POSITION:
            P[off:off + 3] = pl
        elif op in (abi.GOAL_ORIENTATION, abi.GOAL_POSE):
            qo = [ql, -ql, orc_free_quat_mul(ql, (1.0, 0.0, 0.0, 0.0)), orc_free_quat_mul(ql, (np.sin(1e-6), 0.0, 0.0, np.cos(1e-6)))][int(rng.integers(4))]
            if op == abi.GOAL_POSE:
                P[off:off + 3], P[off + 3:off + 7] = pl, qo
            else:
                P[off:off + 4] = qo
        elif op == abi.GOAL_LOOK_AT:
            a = np.asarray(Rl @ np.asarray(P[off:off + 3], dtype=LD), dtype=np.float64)
            P[off + 3:off + 6] = pl + a / np.linalg.norm(a) * 0.5 + tiny * np.array([1.0, -1.0, 0.5])
        elif op in (abi.GOAL_MAX_DISTANCE, abi.GOAL_MIN_DISTANCE):
            P[off + 3] = float(np.linalg.norm(pl - P[off:off + 3])) + tiny
        elif op == abi.GOAL_LINE:
            P[off:off + 3] = pl + P[off + 3:off + 6] * float(rng.normal())
        elif op == abi.GOAL_PLANE:
            nrm = P[off + 3:off + 6]
            P[off:off + 3] = pl + np.cross(nrm, robot_gen.unit(rng, 3)) * 0.3
        elif op == abi.GOAL_SIDE:
            a = np.asarray(Rl @ np.asarray(P[off:off + 3], dtype=LD), dtype=np.float64)
            d = np.cross(a, robot_gen.unit(rng, 3))
            P[off + 3:off + 6] = d / np.linalg.norm(d)
        elif op == abi.GOAL_DIRECTION:
            P[off + 3:off + 6] = np.asarray(Rl @ np.asarray(P[off:off + 3], dtype=LD), dtype=np.float64)
        elif op == abi.GOAL_CONE:
            v = np.asarray(Rl @ np.asarray(P[off + 4:off + 7], dtype=LD), dtype=np.float64)
            dirn = P[off + 7:off + 10]
            ang = float(np.arccos(np.clip(v @ dirn / np.linalg.norm(v) / np.linalg.norm(dirn), -1, 1)))
            P[off + 10] = ang + (np.spacing(ang) * int(rng.integers(-4, 5)) if k else 0.0)
            if k == 2:
                P[off:off + 3] = pl
    return P


def orc_free_quat_mul(a, b):
    return np.asarray(np_goals.qmul(np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)), dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# (a) function level

def function_level(case, h, n, rng, stats, n_edge=8, n_tables=3):
    """eval_fk, eval_fitness (exact and linear), eval_approximator and eval_check of handle h against long double, on n random configurations and n_edge
    edge configurations with edge goal parameters"""
    t = h.template if hasattr(h, "template") else case.template()
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    m = case.model
    tag = repr(case)
    seed = robot_gen.sample_configurations(m, rng, 1)[0]
    X = np.vstack([robot_gen.sample_configurations(m, rng, n), edge_configurations(case, pr, rng, max(n // 4, 1))])
    genes = X[:, pr.active]
    b = Bounds(pr, pr.full(seed, genes).astype(np.float64))
    R, p = pr.frames(seed, genes)
    # FK
    dev = device_frames(h, seed, genes)
    for l in set(pr.tips):
        ep = np.linalg.norm(dev[l][0] - np.asarray(p[l], dtype=np.float64), axis=1)
        qr = quat_from_rot_batch(R[l])
        qd = np.asarray(dev[l][1], dtype=LD)
        eq = np.asarray(np.minimum(np.linalg.norm(qd - qr, axis=1), np.linalg.norm(qd + qr, axis=1)), dtype=np.float64)
        for what, err, bound in (("fk_p", ep, b.dp(l)), ("fk_q", eq, b.dq(l))):
            r = stats.ratio(what, err, bound, tag)
            assert r <= 1.0, "%s: %s of link %d off by %.3g, bound %.3g (ratio %.3g) at row %d" % (tag, what, l, err[np.argmax(err / bound)], bound[np.argmax(err / bound)], r, int(np.argmax(err / bound)))
    # exact fitness, random goal parameters of the template
    params = t.pack_params()
    fitness_against(case, h, pr, b, seed, params, genes, (R, p), stats, "cost")
    # ... and the edges: one configuration at a time, each with goals put on their edges for it
    E = edge_configurations(case, pr, rng, n_edge)
    for i in range(n_edge):
        g1 = E[i:i + 1, pr.active]
        b1 = Bounds(pr, pr.full(seed, g1).astype(np.float64))
        P1 = edge_params(case, pr, params, seed, g1[0], rng)
        fitness_against(case, h, pr, b1, seed, P1, g1, pr.frames(seed, g1), stats, "cost_edge")
        check_against(case, h, pr, b1, seed, P1, g1, stats, [solve_params(), solve_params(dpos=0.05, drot=5.0, dtwist=-1.0)])
    # approximator tables and linearised fitness
    for i in range(n_tables):
        base = genes[i]
        tb_d, dl_d = h.approximator(seed, base)
        tb_l, dl_l = pr.approximator(seed, base)
        for ti, tl in enumerate(pr.tips):
            ti_d = tip_index(h)[tl]
            sgn = 1.0 if np.dot(tb_d[ti_d, 3:], np.asarray(tb_l[ti, 3:], dtype=np.float64)) >= 0 else -1.0  # (the device's quaternion sign)
            for k, v in enumerate(pr.active):
                lk = var_link(m, int(v))
                floating = m.joint_type[lk] in (abi.JOINT_FLOATING, abi.JOINT_PLANAR)
                bi = Bounds(pr, pr.full(seed, base[None]).astype(np.float64))
                dqv = bi.dq(tl)[0]
                if floating:
                    bound = (C * U * (bi.m[tl] + 1) * (bi.lam[tl][0] + 1) + 4 * np.sqrt(2 * C * U * (bi.m[tl] + 1))) / 1e-5
                else:
                    fac = sum(abs(float(pr.follow_factor(j, lk))) for j in robot_gen.chain_of(m, tl))
                    bound = dqv * (bi.lam[tl][0] + 1) * max(fac, 1.0) * 2
                want = np.asarray(dl_l[ti, k], dtype=np.float64)
                want[3:] *= sgn
                err = np.abs(dl_d[ti_d, k] - want).max()
                r = stats.ratio("table_float" if floating else "table", err, bound, tag)
                assert r <= 1.0, "%s: approximator column of gene %d (%s) for tip link %d off by %.3g, bound %.3g: device %s, long double %s" % (
                    tag, k, m.variable_names[v], tl, err, bound, dl_d[ti_d, k], want)
        near = base + 0.02 * rng.normal(size=(max(n // 8, 4), len(pr.active)))
        lf = pr.linear_frames(tb_l, dl_l, base, near)
        pa, _ = h.fitness(abi.FK_LINEAR, seed, params, near, base)
        lc = pr.costs(seed, params, near, tip_frames=lf)
        bl = Bounds(pr, pr.full(seed, near).astype(np.float64))
        dp, dq = {}, {}
        dv = np.abs(near - base[None])
        for ti, tl in enumerate(pr.tips):
            tabs = np.zeros(len(pr.active))
            for k, v in enumerate(pr.active):
                lk = var_link(m, int(v))
                tabs[k] = (C * U * (bl.m[tl] + 1) * (bl.lam[tl][0] + 1) + 4 * np.sqrt(2 * C * U * (bl.m[tl] + 1))) / 1e-5 \
                    if m.joint_type[lk] in (abi.JOINT_FLOATING, abi.JOINT_PLANAR) else 2 * bl.dq(tl)[0] * (bl.lam[tl][0] + 1) * 4
            mag = np.abs(np.asarray(dl_l[ti], dtype=np.float64)).max(axis=1)
            dp[tl] = bi.dp(tl)[0] + dv @ tabs + C * U * (dv @ mag)
            dq[tl] = bi.dq(tl)[0] + dv @ tabs + C * U * (dv @ mag)
        for l in pr.tips:
            dp.setdefault(l, 0.0)
        sec = np.array([g.isSecondary() for g in t.goals])
        bound = cost_bounds(pr, params, {l: np.asarray(lf[l][0], dtype=np.float64) for l in lf}, {l: np.asarray(lf[l][1], dtype=np.float64) for l in lf},
                            dp, dq, lc, near, seed)[:, ~sec].sum(axis=1)
        want = np.asarray(lc[:, ~sec].sum(axis=1), dtype=np.float64)
        err = np.abs(pa - want)
        r = stats.ratio("linear", err, bound, tag)
        assert r <= 1.0, "%s: linearised primary fitness off by %.3g, bound %.3g (row %d)" % (tag, err[np.argmax(err / bound)], bound[np.argmax(err / bound)], int(np.argmax(err / bound)))
    # success test on random configurations, and near the goal (as parity_cases.success_check_near_goal draws it)
    check_against(case, h, pr, b, seed, params, genes, stats, [solve_params(), solve_params(dpos=0.05, drot=5.0, dtwist=-1.0),
                                                                 solve_params(dpos=0.3, drot=-1.0, dtwist=0.2)])


def var_link(m, v):
    for l in range(m.n_links):
        f = m.joint_first_variable[l]
        if f >= 0 and f <= v < f + abi.JOINT_VAR_COUNT[m.joint_type[l]]:
            return l
    raise AssertionError(v)


def fitness_against(case, h, pr, b, seed, params, genes, frames, stats, what):
    R, p = frames
    pa, sa = h.fitness(abi.FK_EXACT, seed, params, genes)
    lc = pr.costs(seed, params, genes, frames=frames)
    q = {l: np.asarray(quat_from_rot_batch(R[l]), dtype=np.float64) for l in set(pr.tips)}
    pp = {l: np.asarray(p[l], dtype=np.float64) for l in set(pr.tips)}
    bound = cost_bounds(pr, params, pp, q, {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, lc, genes, seed)
    sec = np.array([g.isSecondary() for g in pr.template.goals])
    for got, mask, name in ((pa, ~sec, "primary"), (sa, sec, "secondary")):
        want = np.asarray(lc[:, mask].sum(axis=1), dtype=np.float64)
        bnd = bound[:, mask].sum(axis=1) + C * U * want
        err = np.abs(got - want)
        r = stats.ratio(what, err, np.maximum(bnd, 1e-300), repr(case))
        if r > 1.0:
            i = int(np.argmax(err / np.maximum(bnd, 1e-300)))
            raise AssertionError("%s: %s fitness off by %.3g, bound %.3g (row %d); the goal: %s" % (repr(case), name, err[i], bnd[i], i,
                                                                                                        which_goal(case, h, pr, seed, params, genes[i:i + 1], frames, bound[i], i)))


def which_goal(case, h, pr, seed, params, genes, frames, bound_row, row):
    """one template of one goal per goal of the case, on the same library: the first goal whose own fitness leaves its bound"""
    from bio_ik_amd import ProblemTemplate
    lc = pr.costs(seed, params, genes)
    for k, (goal, off) in enumerate(zip(case.goals, pr.template.param_offsets)):
        try:
            t1 = ProblemTemplate(case.model, "g", [goal], fixed_joints=case.fixed)
            h1 = solver.HipSolver(t1, lib=h.L)
        except (solver.BioIKError, orc.OracleError, KeyError):  # (a goal alone may not make a problem)
            continue
        if not np.array_equal(h1.active_variables, h.active_variables):
            continue
        P1 = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[goal.opcode]])
        a, s = h1.fitness(abi.FK_EXACT, seed, P1, genes)
        got = (s if goal.isSecondary() else a)[0]
        if abs(got - float(lc[0, k])) > bound_row[k]:
            return "#%d %s: device %.17g, long double %.17g, bound %.3g" % (k, type(goal).__name__, got, float(lc[0, k]), bound_row[k])
    return "(no single goal leaves its bound: the sum's order)"


def check_against(case, h, pr, b, seed, params, genes, stats, plist):
    """eval_check against np_goals.Problem.check: equal flags except where a tested quantity lies within its bound of its threshold"""
    R, p = pr.frames(seed, genes)
    lc = None
    for sp in plist:
        dpos, drot, dtwist = thresholds(sp)
        ok, vals = pr.check(seed, params, genes, dpos, drot, dtwist, frames=(R, p))
        got = h.check(sp, seed, params, genes).astype(bool)
        band = np.zeros(len(ok), dtype=bool)
        for v, th, kind, where in vals:
            v = np.asarray(v, dtype=np.float64)
            if kind == "cost":
                if lc is None:
                    lc = pr.costs(seed, params, genes, frames=(R, p))
                    q = {l: np.asarray(quat_from_rot_batch(R[l]), dtype=np.float64) for l in set(pr.tips)}
                    cb = cost_bounds(pr, params, {l: np.asarray(p[l], dtype=np.float64) for l in set(pr.tips)}, q, {l: b.dp(l) for l in b.m},
                                     {l: b.dq(l) for l in b.m}, lc, genes, seed)
                bnd = cb[:, where]
            else:
                dp, dq = b.dp(where), b.dq(where)
                if kind == "pos":
                    bnd = dp
                elif kind == "rot":
                    x = np.cos(np.radians(v) / 2)
                    dx = 2 * dq
                    bnd = np.degrees(2 * dx / np.maximum(np.sqrt(np.maximum(1 - x * x, 0)), np.sqrt(dx)))
                elif kind == "tw_lin":
                    bnd = dp + 2 * dq * np.linalg.norm(np.asarray(p[where], dtype=np.float64), axis=1)
                else:
                    bnd = 4 * dq + 2e-6  # (KDL's GetRot takes a rotation within 1e-6 of symmetric as none at all: a component of up to 1e-6 may read 0)
            band |= np.abs(v - float(th)) <= bnd
        stats.rows += len(ok)
        stats.band += int(band.sum())
        bad = (ok != got) & ~band
        assert not bad.any(), "%s: success test differs outside the band at rows %s (device %s, long double %s)" % (repr(case), np.nonzero(bad)[0][:8], got[bad][:8], ok[bad][:8])


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# (b) whole solves bit for bit

# (mode, fk, population, islands, switches, schedule): the plans the cases cycle through; the launcher's own choice where switches are empty
PLANS = [
    ("bio2", abi.FK_EXACT, 8, 1, {}, "latency"),
    ("bio2_memetic", abi.FK_LINEAR, 16, 2, {}, "latency"),
    ("bio2_memetic_l", abi.FK_EXACT, 33, 1, {}, "latency"),
    ("bio2", abi.FK_LINEAR, 128, 1, {}, "latency"),
    ("bio2_memetic", abi.FK_EXACT, 129, 3, {}, "latency"),
    ("bio2", abi.FK_EXACT, 512, 1, {}, "latency"),
    ("bio2", abi.FK_EXACT, 128, 1, {}, "throughput"),
    ("bio2_memetic", abi.FK_EXACT, 70, 1, {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_COLUMNLESS": "2", "BIOIK_SOLVE_FOUR_WAVES": "1"}, "latency"),
    ("bio2", abi.FK_EXACT, 33, 2, {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_SPECIES_PARALLEL": "1", "BIOIK_SOLVE_COLUMNLESS": "2"}, "latency"),
    ("bio2", abi.FK_EXACT, 65, 1, {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_SPECIES_PARALLEL": "1", "BIOIK_SOLVE_COLUMNLESS": "2",
                                   "BIOIK_SOLVE_THREE_WAVES": "1"}, "latency"),
    ("bio2_memetic", abi.FK_EXACT, 16, 1, {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_COLUMNLESS": "1"}, "latency"),
    ("bio2", abi.FK_EXACT, 24, 4, {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_COLUMNLESS": "0"}, "latency"),
    ("bio2", abi.FK_EXACT, 40, 1, {"BIOIK_SOLVE_GENERAL": "1"}, "latency"),
    ("bio2_memetic", abi.FK_EXACT, 200, 2, {"BIOIK_SOLVE_HELPED": "0"}, "latency"),
    ("bio2", abi.FK_LINEAR, 31, 1, {}, "latency"),
    ("gd", abi.FK_EXACT, 1, 1, {}, "latency"),
    ("gd_r", abi.FK_EXACT, 1, 2, {}, "latency"),
    ("gd_c", abi.FK_EXACT, 1, 1, {}, "latency"),
    ("jac", abi.FK_EXACT, 1, 3, {}, "latency"),
]


# ... and for serial chains without secondary goals, the kernels compiled for one lane mapping: the helped build, the 128-register build, the dense kernel
SERIAL_PLANS = [
    ("bio2", abi.FK_EXACT, 128, 1, {}, "latency"),
    ("bio2_memetic", abi.FK_EXACT, 131, 2, {}, "latency"),
    ("bio2", abi.FK_EXACT, 200, 1, {"BIOIK_SOLVE_HELPED": "0"}, "latency"),
    ("bio2", abi.FK_EXACT, 70, 1, {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_COLUMNLESS": "2", "BIOIK_SOLVE_FOUR_WAVES": "1"}, "latency"),
    ("bio2", abi.FK_EXACT, 128, 1, {}, "throughput"),
    ("bio2_memetic", abi.FK_EXACT, 256, 3, {}, "throughput"),
]


def whole_solve(case, h, o, plan, report, monkeypatch, n=2, steps=2, nan_ok=True):
    """parity_cases.trajectory with NaN equal to NaN (a goal met exactly makes the line search divide 0 by 0, on both sides alike): all four outputs.
    Returns the kernels that ran."""
    mode, fk, pop, islands, env, schedule = plan
    t = case.template()
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, n, seed=case.seed)
    kw = {"population": max(pop, 2), "max_steps": steps if not mode.startswith(("gd", "jac")) else 6, "random_seed": 11, "mode": mode, "fk_mode": fk,
          "islands": islands, "schedule": abi.SCHEDULE_BY_NAME[schedule]}
    p = abi.default_solve_params(**kw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        report.read()
        got = h.solve_batch(p, seeds, params)
        ran = set(report.kernels(report.read()))
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
    want = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=4)
    for name, a, b in zip(("solutions", "fitness", "success", "steps"), want, got):
        assert np.array_equal(a, b, equal_nan=nan_ok), "%s: whole solves differ in %s under %s (kernels %s): oracle %s, device %s" % (
            repr(case), name, plan, sorted(ran), np.asarray(a).ravel()[:6], np.asarray(b).ravel()[:6])
    return ran


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# (c) the result contract

def result_contract(case, h, n, rng, stats, islands=1, island_sync=0, steps=12, pop=16):
    """solves under the default program, goals in any order: goals put on their edges (edge_params) for the long-double FK of a random target configuration,
    seeds at random or near the target.  For every row:
      - inactive variables are the seed's, bit for bit; bounded variables lie within [min, max], the others within +-BIOIK_SINCOS_DOMAIN; steps in [1, max_steps];
      - fitness is the device's own eval_fitness of the returned solution, bit for bit: the primary term, plus the secondary term where the query
        succeeded and the template has secondary goals (ik_parallel.h:222-246, solve_epilogue) -- or DBL_MAX with solution = seed where nothing improved;
      - it agrees with the long-double cost of the solution within the bound;
      - success implies the long-double success test passes, up to the band."""
    t = case.template()
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    m = case.model
    X = robot_gen.sample_configurations(m, rng, 2 * n, odd_norms=False)  # (seeds within the variables' bounds)
    seeds, targets = X[:n], X[n:]
    near = rng.random(n) < 0.5  # (half the queries start near their target: solves that succeed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    seeds[near] = np.clip(targets[near] + 0.02 * rng.normal(size=(int(near.sum()), m.n_variables)), lo, hi)
    inactive = np.setdiff1d(np.arange(m.n_variables), pr.active)
    seeds[:, inactive] = targets[:, inactive]
    seeds = robot_gen.normalise_quaternions(m, seeds)
    base = t.pack_params()
    params = np.stack([edge_params(case, pr, base, targets[i], targets[i, pr.active], rng) for i in range(n)])
    sp = abi.default_solve_params(population=pop, max_steps=steps, random_seed=int(rng.integers(1 << 30)), islands=islands, island_sync=island_sync,
                                  mode="bio2_memetic", fk_mode=abi.FK_EXACT)
    sol, fit, suc, stp = h.solve_batch(sp, seeds, params)
    assert np.array_equal(sol[:, inactive], seeds[:, inactive]), "%s: an inactive variable moved" % repr(case)
    genes = sol[:, pr.active]
    inside = ((genes >= lo[pr.active]) & (genes <= hi[pr.active])) | ~pr.bounded
    assert inside.all(), "%s: a bounded variable outside [min, max] at rows %s" % (repr(case), np.nonzero(~inside.all(axis=1))[0][:6])
    # (a variable without bounds: inside the domain on which the shared sincos is right -- a line-search candidate at or beyond it is no candidate, quirk Q7)
    domain = solver.sincos_domain(h.L)
    assert (np.abs(genes[:, ~pr.bounded]) < domain).all(), "%s: a variable without bounds of magnitude >= %g came back" % (repr(case), domain)
    assert ((stp >= 1) & (stp <= steps)).all(), "%s: steps %s outside [1, %d]" % (repr(case), stp, steps)
    has_sec = any(g.isSecondary() for g in t.goals)
    kept = fit == DBL_MAX
    assert np.array_equal(sol[kept], seeds[kept]), "%s: fitness DBL_MAX but the solution is not the seed" % repr(case)
    sec = np.array([g.isSecondary() for g in t.goals])
    for i in np.nonzero(~kept)[0]:
        pa, sa = h.fitness(abi.FK_EXACT, seeds[i], params[i], genes[i:i + 1])
        expect = pa[0] + sa[0] if (suc[i] and has_sec) else pa[0]
        assert fit[i] == expect, "%s: row %d (success %d): reported fitness %.17g, eval_fitness of the solution %.17g + %.17g" % (
            repr(case), i, suc[i], fit[i], pa[0], sa[0])
        g1 = genes[i:i + 1]
        fr = pr.frames(seeds[i], g1)
        b = Bounds(pr, pr.full(seeds[i], g1).astype(np.float64))
        lc = pr.costs(seeds[i], params[i], g1, frames=fr)
        q = {l: np.asarray(quat_from_rot_batch(fr[0][l]), dtype=np.float64) for l in set(pr.tips)}
        cb = cost_bounds(pr, params[i], {l: np.asarray(fr[1][l], dtype=np.float64) for l in set(pr.tips)}, q, {l: b.dp(l) for l in b.m},
                         {l: b.dq(l) for l in b.m}, lc, g1, seeds[i])[0]
        mask = ~sec | (bool(suc[i]) and has_sec)
        want = float(lc[0, mask].sum())
        err = abs(fit[i] - want)
        bnd = cb[mask].sum() + C * U * abs(want)
        r = stats.ratio("contract_cost", err, max(bnd, 1e-300), repr(case))
        assert r <= 1.0, "%s: row %d fitness %.17g, long double %.17g, bound %.3g" % (repr(case), i, fit[i], want, bnd)
        if suc[i]:
            check_against(case, h, pr, b, seeds[i], params[i], g1, stats, [sp])
    return int(suc.sum()), int(kept.sum()), int(suc.sum()) if has_sec else 0


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# (d) joint angles up to the end of the sincos's domain

HUGE_ROWS = 64


def huge_angle_cases():
    """One continuous joint; a chain of three continuous joints with oblique axes and rotated origins; that chain with a follower of factor -1.5 behind it; that
    chain with its middle joint held fixed (an INACTIVE continuous variable on the tip's chain: it keeps the seed's value, which huge_angle_level puts at 1e10).
    One tip on a fixed link behind the last joint, one PoseGoal on it."""
    from bio_ik_amd import PoseGoal, RobotModel

    def chain(name, n_joints, follower=False):
        m = RobotModel(name)
        m.add_link("l0")
        spec = [((0.1, 0.05, 0.2), (0.3, -0.2, 0.5), (0.3, -0.5, 0.8)), ((0.25, -0.1, 0.05), (-0.4, 0.7, 0.1), (-0.6, 0.2, 0.7)), ((0.05, 0.2, -0.15), (0.9, 0.1, -0.6), (0.5, 0.7, -0.4))]
        joints = []
        for k in range(n_joints):
            m.add_link("l%d" % (k + 1), "l%d" % k, "j%d" % (k + 1), "continuous", xyz=spec[k][0], rpy=spec[k][1], axis=spec[k][2], velocity=1.0 + k)
            joints.append("j%d" % (k + 1))
        last = "l%d" % n_joints
        if follower:  # (offset 0: the follower's angle, -1.5 x the leader's, is then a double wherever the leader's last two mantissa bits are clear)
            m.add_link("lf", last, "jf", "continuous", xyz=(0.1, -0.05, 0.1), rpy=(0.2, 0.3, -0.7), axis=(0.1, -0.9, 0.4), velocity=2.0, mimic=("j2", -1.5, 0.0))
            joints.append("jf")
            last = "lf"
        m.add_link("tool", last, "tool_joint", "fixed", xyz=(0.15, -0.1, 0.2), rpy=(0.3, 0.3, 0.3))
        m.add_group("g", joints=joints, tips=["tool"])
        return m, joints

    out = []
    for k, (name, n_joints, follower, fixed) in enumerate((("turn1", 1, False, []), ("turn3", 3, False, []), ("turn3_follower", 3, True, []), ("turn3_held", 3, False, ["j2"]))):
        m, joints = chain(name, n_joints, follower)
        goals = [PoseGoal("tool", (0.3, -0.2, 0.5), (0.1, -0.3, 0.2, 0.9))]
        out.append(robot_gen.Case(9000 + k, m, joints, [m.link_index("tool")], goals, fixed, True, None))
    return out


def huge_angles(rng, domain, shape):
    """log-uniform in 1e5 ... the domain, both signs, the last two mantissa bits clear (so that -1.5 x the value, a follower's angle, is a double also where it
    falls into the next binade: the comparison is about the sincos, not about an argument that either side has rounded); the first rows: 6.8e9 and 2e10, whose half angles lie just past 2^31 pi / 2 = 3.37e9"""
    x = np.exp(rng.uniform(np.log(1e5), np.log(domain), shape)) * rng.choice([-1.0, 1.0], shape)
    x = np.minimum(np.abs(x), np.nextafter(domain, 0.0)) * np.sign(x)
    x[0], x[1], x[2], x[3] = 6.8e9, 2e10, -6.8e9, -2e10
    x = (x.view(np.uint64) & ~np.uint64(3)).view(np.float64)
    assert np.all((np.abs(x) >= 1e5) & (np.abs(x) < domain))
    return x


def huge_angle_level(case, h, o, stats, exact):
    """eval_fk, eval_fitness and eval_check of handle h at HUGE_ROWS configurations whose continuous joints stand at 1e5 ... BIOIK_SINCOS_DOMAIN rad, against long
    double to C u (m + 1) Lambda: the bounds of `Bounds` WITHOUT the Theta term, which is vacuous here (u |theta| is 1e-2 at 1e14) -- the measured error of the
    shared sincos is absolute and flat over its domain (bioik_sincos.h), and a half angle theta / 2 is exact.  Under the exact program eval_fk is the oracle's
    (arithmetic mode 1) bit for bit."""
    t = h.template
    m = case.model
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    domain = solver.sincos_domain(h.L)
    rng = np.random.default_rng(case.seed)
    seed = robot_gen.sample_configurations(m, rng, 1)[0]
    inactive = np.setdiff1d(np.arange(m.n_variables), pr.active)
    seed[inactive] = 1e10  # (every variable of these robots is a continuous joint's: the held joint's stays, a follower's is overwritten by its leader's)
    genes = huge_angles(rng, domain, (HUGE_ROWS, len(pr.active)))
    tag = repr(case) + (" exact" if exact else " folded")
    b = Bounds(pr, pr.full(seed, genes).astype(np.float64))
    assert all(np.all(th >= 1e5 / np.pi) for th in b.theta.values())  # (what the Theta term would have allowed: 1e5 and more times the bound below)
    b.theta = {l: np.zeros(HUGE_ROWS) for l in b.theta}
    R, p = pr.frames(seed, genes)
    dev = device_frames(h, seed, genes)
    for l in set(pr.tips):
        ep = np.linalg.norm(dev[l][0] - np.asarray(p[l], dtype=np.float64), axis=1)
        qr = quat_from_rot_batch(R[l])
        qd = np.asarray(dev[l][1], dtype=LD)
        eq = np.asarray(np.minimum(np.linalg.norm(qd - qr, axis=1), np.linalg.norm(qd + qr, axis=1)), dtype=np.float64)
        for what, err, bound in (("huge_fk_p", ep, b.dp(l)), ("huge_fk_q", eq, b.dq(l))):
            r = stats.ratio(what, err, bound, tag)
            i = int(np.argmax(err / bound))
            assert r <= 1.0, "%s: %s off by %.3g, bound %.3g (ratio %.3g) at row %d, genes %s" % (tag, what, err[i], bound[i], r, i, genes[i])
    if exact:
        want = o.fk_genes(seed, genes)
        got = h.fk_genes(seed, genes)
        differ = np.nonzero((want != got).any(axis=(1, 2)))[0]
        assert differ.size == 0, "%s: eval_fk differs from the oracle at rows %s, genes %s: oracle %s, device %s" % (tag, differ[:6], genes[differ[0]], want[differ[0]], got[differ[0]])
    # the PoseGoal on the pose of row 0 (so that one row passes the success test), every row's cost and success decision
    params = edge_params(case, pr, t.pack_params(), seed, genes[0], rng)
    fitness_against(case, h, pr, b, seed, params, genes, (R, p), stats, "huge_cost")
    before = stats.rows
    check_against(case, h, pr, b, seed, params, genes, stats, [solve_params(), solve_params(dpos=0.05, drot=5.0, dtwist=-1.0)])
    assert stats.rows == before + 2 * HUGE_ROWS
    ok = pr.check(seed, params, genes, *thresholds(solve_params(dpos=0.05, drot=5.0, dtwist=-1.0)), frames=(R, p))[0]
    assert ok[0] and not ok.all()


def huge_angle_levels(case, make_solver, stats):
    """(d) under both joint programs"""
    for exact in (False, True):
        with program(exact):
            made = make_or_refuse(case, make_solver)
        assert made is not None, repr(case)
        h, o = made
        assert np.array_equal(h.active_variables, o.active_variables) and np.array_equal(h.tip_links, o.tip_links), repr(case)
        assert (len(h.active_variables) < case.model.n_variables) == bool(case.fixed or "jf" in case.joints), repr(case)
        huge_angle_level(case, h, o, stats, exact)


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# the drivers of the two test files

def make_or_refuse(case, make_solver):
    """(handle, oracle) of the case, or None where both refuse it.  The device refuses exactly what the oracle refuses and the shapes of
    robot_gen.expected_refusal; the oracle takes those."""
    t = case.template()
    try:
        o = orc.Oracle(t)
    except orc.OracleError as e:
        try:
            make_solver(t)
        except solver.BioIKError:
            return None
        raise AssertionError("%s: the oracle refuses (%s), the device does not" % (repr(case), e))
    try:
        h = make_solver(t)
    except solver.BioIKError as e:
        assert case.refusal is not None or (case.may_refuse is not None and case.may_refuse in str(e)), \
            "%s: the device refuses a shape it supports: %s" % (repr(case), e)
        assert e.code == abi.ERR_UNSUPPORTED, (repr(case), e)
        return None
    assert case.refusal is None, "%s: the device takes a shape it must refuse (%s)" % (repr(case), case.refusal)
    if o.D == 0:
        return None
    return h, o


def function_levels(case, make_solver, n, stats, n_edge):
    """(a) under both joint programs; returns the number of programs compared"""
    done = 0
    for exact in (False, True):
        with program(exact):
            made = make_or_refuse(case, make_solver)
        if made is None:
            return done
        h, o = made
        assert np.array_equal(h.active_variables, o.active_variables) and np.array_equal(h.tip_links, o.tip_links), repr(case)
        function_level(case, h, n, np.random.default_rng(case.seed * 7 + exact), stats, n_edge=n_edge)
        done += 1
    return done


def whole_solves(case, make_solver, report, monkeypatch, k, plans=PLANS, exact=True):
    """(b): the k-th plan of `plans` (and the next one) on a goal list in walk order, under BIOIK_COMPILE_EXACT=1 (exact) or under the default program,
    which folds the trees of random_case(plain=True) exactly; returns the kernels that ran"""
    if not case.walk or any(g.opcode == abi.GOAL_BALANCE for g in case.goals):  # (the device sums the centre of mass in walk order: to rounding)
        return set()
    with program(exact):
        made = make_or_refuse(case, make_solver)
    if made is None:
        return set()
    h, o = made
    ran = set()
    for j in (k, k + 1):
        ran |= whole_solve(case, h, o, plans[j % len(plans)], report, monkeypatch)
    return ran
