"""Base links (bioik_problem_desc::goal_base_link, include/bioik_hip.h: BASE LINKS) on the library under test: the GPU suite (tests/test_gpu_base_link.py) and
the host simulator (tests/test_hostsim_base_link.py) run these cases.  `make_solver(template)` makes a bio_ik_amd.solver.HipSolver of the library under test.

The pin is the rule restated in long double from its definition, on the long-double forward kinematics of tests/np_fk.py -- not the oracle (it does not know
the field) and not the kernel.  With A = (pA, qA) the base link's frame and B = (pB, qB) the goal link's frame,

    R.q = conj(qA) (x) qB          R.p = rotate(conj(qA), -pA) + rotate(conj(qA), pB)          (nothing normalised)

the cost is np_goals.link_cost on R and the success test np_goals.Problem.check on R (as a rotation matrix: A^T B, A^T (pB - pA)).

Error bound, built like those of tests/random_robot_cases.py and tests/touch_cases.py (the same C and U, the same FK bounds dp / dq of a tip -- here of BOTH tips --
and the same `rot` of a vector rotated by a quaternion known to dq).  With nA = |qA|, nB = |qB| (1 for exact FK, near 1 for linearised frames):

    |dR.q| <= nB dqA + nA dqB + C U nA nB                                  a product of two quaternions, each known to its dq, and its own roundings
    |dR.p| <= amp (dpA + dpB) + (rotA + C U amp) (|pA| + |pB|)             amp = 1 + 3 nA^2 bounds |rotate(q, v)| / |v| of the polynomial form
                                                                            v + 2 w (u x v) + 2 u x (u x v); rotA = 2 dqA (1 + nA^2) per unit length.  The two
                                                                            positions are rotated one by one, so the roundings scale with |pA| + |pB|, not with
                                                                            |pB - pA|

and R with (dR.p, dR.q) takes the place of a tip's frame with (dp, dq) in random_robot_cases.cost_bounds and in the bands of the success test
(random_robot_cases.check_against).  The check is error <= bound; -s prints the worst ratios."""
import types

import numpy as np

import np_goals
import random_robot_cases as rr
import touch_cases as tc
from bio_ik_amd import (ConeGoal, DirectionGoal, LineGoal, LookAtGoal, MaxDistanceGoal, MinDistanceGoal, OrientationGoal, PlaneGoal, PoseGoal, PositionGoal,
                        ProblemTemplate, SideGoal, TouchGoal, abi, pr2_like, solver)
from np_fk import LD, quat_from_rot_batch
from tools import robot_gen

C, U = rr.C, rr.U
RW, LW = "r_wrist_roll_link", "l_wrist_roll_link"
RE, LE = "r_elbow_flex_link", "l_elbow_flex_link"
FRAME_GOALS = (abi.GOAL_POSITION, abi.GOAL_ORIENTATION, abi.GOAL_POSE)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------
def conj(q):
    return np.asarray(q, dtype=LD) * np.array([-1, -1, -1, 1], dtype=LD)


def relative(pA, qA, pB, qB):
    """R = concat(invert(A), B) for frames (n, 3), (n, 4): long double, the formula as it stands"""
    pA, qA, pB, qB = (np.asarray(a, dtype=LD) for a in (pA, qA, pB, qB))
    c = conj(qA)
    return np_goals.qrot(c, -pA) + np_goals.qrot(c, pB), np_goals.qmul(c.T, qB.T).T


def relative_bound(pA, qA, pB, qB, dpA, dqA, dpB, dqB):
    """(|dR.p|, |dR.q|) of the module's docstring"""
    pA, qA, pB, qB = (np.asarray(a, dtype=np.float64) for a in (pA, qA, pB, qB))
    nA, nB = np.linalg.norm(qA, axis=1), np.linalg.norm(qB, axis=1)
    amp = 1 + 3 * nA * nA
    rotA = 2 * dqA * (1 + nA * nA)
    return amp * (dpA + dpB) + (rotA + C * U * amp) * (np.linalg.norm(pA, axis=1) + np.linalg.norm(pB, axis=1)), nB * dqA + nA * dqB + C * U * nA * nB


def base_of(g):
    b = getattr(g, "base_link_name", None)
    return b() if b else None


def goal_frame(t, g, frames, dp, dq):
    """the frame goal g reads, as (p, q, dp, dq): its link's, or R for a based goal"""
    link = t.model.link_index(g.link_name())
    (pB, qB), dpB, dqB = frames[link], dp[link], dq[link]
    if base_of(g) is None:
        return pB, qB, dpB, dqB
    base = t.model.link_index(base_of(g))
    (pA, qA), dpA, dqA = frames[base], dp[base], dq[base]
    p, q = relative(pA, qA, pB, qB)
    d_p, d_q = relative_bound(pA, qA, pB, qB, dpA, dqA, dpB, dqB)
    return p, q, d_p, d_q


def one_goal(t, g):
    """what random_robot_cases.cost_bounds and np_goals.Problem read of a problem, for the single goal g"""
    return types.SimpleNamespace(model=t.model, template=types.SimpleNamespace(model=t.model, goals=[g], param_offsets=[0]))


def costs_and_bounds(t, params, frames, dp, dq):
    """weighted cost (n, n_goals) in long double and its bound, for frames {link: (p, q)} known to dp / dq {link: (n,)}"""
    n = next(iter(frames.values()))[0].shape[0]
    cost = np.zeros((n, len(t.goals)), dtype=LD)
    bound = np.zeros((n, len(t.goals)))
    for k, (g, off) in enumerate(zip(t.goals, t.param_offsets)):
        P = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[g.opcode]], dtype=np.float64)
        link = t.model.link_index(g.link_name())
        p, q, d_p, d_q = goal_frame(t, g, frames, dp, dq)
        cost[:, k] = np_goals.link_cost(g.opcode, np.asarray(P, dtype=LD), p, q) * LD(g.getWeight()) ** 2
        bound[:, k] = rr.cost_bounds(one_goal(t, g), P, {link: p}, {link: q}, {link: d_p}, {link: d_q}, cost[:, k:k + 1])[:, 0]
    return cost, bound


def total(cost, bound):
    want = np.asarray(cost.sum(axis=1), dtype=np.float64)
    return want, bound.sum(axis=1) + C * U * want


def exact_frames(pr, seed, genes):
    R, p = pr.frames(seed, genes)
    return {l: (p[l], quat_from_rot_batch(R[l])) for l in set(pr.tips)}, (R, p)


def success_test(t, pr, params, Rp, dpos, drot, dtwist, dp, dq):
    """Problem::checkSolutionActiveVariables with R in place of a based goal's frame, in long double: (ok (n,), band (n,), margins) -- band: some tested quantity lies
    within its error bound of its threshold (the bands of random_robot_cases.check_against, with R's bounds); margins: per tested quantity (value - threshold, bound)"""
    R, p = Rp
    n = p.shape[1]
    frames = {l: (p[l], quat_from_rot_batch(R[l])) for l in set(pr.tips)}
    cost, cbound = costs_and_bounds(t, params, frames, dp, dq)
    ok, band, margins = np.ones(n, dtype=bool), np.zeros(n, dtype=bool), []
    for k, (g, off) in enumerate(zip(t.goals, t.param_offsets)):
        P = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[g.opcode]], dtype=np.float64)
        link = t.model.link_index(g.link_name())
        pg, qg, d_p, d_q = goal_frame(t, g, frames, dp, dq)
        Rg, pgm = R[link], p[link]
        if base_of(g) is not None:  # the definition on rotation matrices: A^T B, A^T (pB - pA)
            A, pA = R[t.model.link_index(base_of(g))], p[t.model.link_index(base_of(g))]
            Rg, pgm = np.einsum("nji,njk->nik", A, Rg), np.einsum("nji,nj->ni", A, pgm - pA)
        Ra, pa = np.zeros_like(R), np.zeros_like(p)
        Ra[link], pa[link] = Rg, pgm
        ok1, vals = np_goals.Problem(one_goal(t, g).template, pr.active, [link]).check(None, P, np.zeros((n, len(pr.active))), dpos, drot, dtwist, frames=(Ra, pa))
        ok &= ok1
        for v, th, kind, _ in vals:
            v = np.asarray(v, dtype=np.float64)
            if kind == "cost":
                bnd = cbound[:, k]
            elif kind == "pos":
                bnd = d_p
            elif kind == "rot":
                x, dx = np.cos(np.radians(v) / 2), 2 * d_q
                bnd = np.degrees(2 * dx / np.maximum(np.sqrt(np.maximum(1 - x * x, 0)), np.sqrt(dx)))
            elif kind == "tw_lin":
                bnd = d_p + 2 * d_q * np.linalg.norm(np.asarray(pg, dtype=np.float64), axis=1)
            else:
                bnd = 4 * d_q + 2e-6  # (KDL's GetRot takes a rotation within 1e-6 of symmetric as none at all, random_robot_cases.check_against)
            band |= np.abs(v - float(th)) <= bnd
            margins.append((v - float(th), bnd))
    return ok, band, margins


# ---- function level -----------------------------------------------------------------------------------------------------------------------------------------
def tool_model():
    """pr2_like with a fixed tool frame behind each wrist (a rotated, offset origin): tips with a constant trailing frame (DevTip::has_e)"""
    m = pr2_like()
    m.add_link("r_tool", RW, "r_tool_joint", "fixed", xyz=(0.18, 0.0, 0.02), rpy=(0.3, -0.2, 0.5))
    m.add_link("l_tool", LW, "l_tool_joint", "fixed", xyz=(0.15, 0.01, 0.0), rpy=(0.0, 0.4, -0.1))
    return m


def held_limit_model():
    """a tree of tools/robot_gen.py (the random robots of tests/random_robot_cases.py) with at least 2 BIOIK_MAX_HELD_FRAMES + 2 moving links, no mimic joint"""
    need = 2 * abi.MAX_HELD_FRAMES + 2
    for s in range(1, 200):
        m, joints, n = robot_gen.random_robot(np.random.default_rng(s), s, big=True, mimic=False)
        moving = [l for l in range(1, n) if m.joint_type[l] in (abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC)]
        branches = len(set(m.link_parent[l] for l in range(1, n))) < n - 1
        if len(moving) >= need and branches:
            m.add_group("g", joints=joints, tips=["l%d" % l for l in moving[:need]])
            return m, ["l%d" % l for l in moving[:need]]
    raise AssertionError("no such tree")


def held_limit_goals(links, pairs):
    """`pairs` based PositionGoals on disjoint pairs of links: as many distinct held frames"""
    rng = np.random.default_rng(pairs)
    return [PositionGoal(links[2 * i], tuple(rng.normal(size=3) * 0.3), weight=0.5 + 0.25 * i, base_link=links[2 * i + 1]) for i in range(pairs)]


def every_opcode(link, base, rng):
    u = lambda k: robot_gen.unit(rng, k)  # noqa: E731
    p = lambda: tuple(rng.normal(size=3) * 0.3)  # noqa: E731
    return [PositionGoal(link, p(), weight=0.7, base_link=base), OrientationGoal(link, u(4), weight=0.5, base_link=base),
            LookAtGoal(link, u(3), p(), weight=0.9, base_link=base), MaxDistanceGoal(link, p(), 0.2, weight=1.1, base_link=base),
            MinDistanceGoal(link, p(), 0.9, weight=0.6, base_link=base), LineGoal(link, p(), u(3), weight=0.8, base_link=base),
            PlaneGoal(link, p(), u(3), weight=1.2, base_link=base), SideGoal(link, u(3), u(3), weight=0.4, base_link=base),
            DirectionGoal(link, u(3), u(3), weight=1.0, base_link=base), ConeGoal(link, u(3), u(3), 0.3, weight=0.5, position=p(), position_weight=0.5, base_link=base)]


def function_cases():
    """name -> (model, group, goals): the smallest shapes at which the holding can go wrong (the walk completes the tips in the order their links are first named,
    a link behind another on one chain after it)"""
    rng = np.random.default_rng(7)
    u4 = lambda: robot_gen.unit(rng, 4)  # noqa: E731
    P1, P2, P3 = (0.1, -0.3, 0.05), (-0.2, 0.25, 0.1), (0.05, 0.1, -0.2)
    out = {}
    m = pr2_like
    # 1. the base reached before the goal's link (the world goal names the right wrist first), and the same two links swapped
    out["base_first"] = (m(), "all", [PositionGoal(RW, (0.6, -0.2, 0.8)), PoseGoal(LW, P1, u4(), base_link=RW)])
    out["base_last"] = (m(), "all", [PositionGoal(RW, (0.6, -0.2, 0.8)), PoseGoal(RW, P1, u4(), base_link=LW)])
    # 2. one base with two goals on different links; two goals with different bases on one link
    out["one_base_two_links"] = (m(), "all", [PoseGoal(LW, P1, u4(), base_link=RW), PositionGoal(LE, P2, weight=0.7, base_link=RW)])
    out["two_bases_one_link"] = (m(), "all", [PositionGoal(RE, (0.4, -0.2, 0.9), weight=0.3), PoseGoal(LW, P1, u4(), base_link=RW), OrientationGoal(LW, u4(), weight=0.8, base_link=RE)])
    # 3. a based goal beside a world goal of the same opcode on one tip; the based PoseGoal as the tip's only goal (beside a world PoseGoal on the base)
    out["beside_world_goal"] = (m(), "all", [PoseGoal(RW, (0.6, -0.2, 0.8), u4()), PoseGoal(LW, (0.5, 0.3, 0.9), u4(), weight=0.6), PoseGoal(LW, P1, u4(), base_link=RW)])
    out["only_goal_of_its_tip"] = (m(), "all", [PoseGoal(RW, (0.6, -0.2, 0.8), u4()), PoseGoal(LW, P1, u4(), base_link=RW)])
    out["only_goal"] = (m(), "all", [PoseGoal(LW, P1, u4(), base_link=RW)])
    # 4. one of every eligible opcode besides Pose with a base, in one problem
    out["every_opcode"] = (m(), "all", every_opcode(LW, RW, rng))
    # 5. a base link with a constant trailing frame; a base link that hangs off the model root without a moving joint (with and without an offset)
    out["base_has_trailing_frame"] = (tool_model(), "all", [PoseGoal("l_tool", P1, u4(), base_link="r_tool"), PositionGoal("r_tool", P3, weight=0.5, base_link=LW)])
    out["base_is_root"] = (m(), "right_arm", [PoseGoal(RW, (0.6, -0.2, 0.8), u4(), base_link="base_footprint"), PositionGoal(RW, (0.6, -0.2, 0.75), weight=0.5, base_link="base_link")])
    # 6. base and link on one serial chain, either way round
    out["elbow_against_wrist"] = (m(), "right_arm", [PoseGoal(RW, P3, u4(), base_link=RE)])
    out["wrist_against_elbow"] = (m(), "right_arm", [PoseGoal(RE, P3, u4(), base_link=RW)])
    # 7. BIOIK_MAX_HELD_FRAMES distinct held frames on a tree
    tree, links = held_limit_model()
    out["held_limit"] = (tree, "g", held_limit_goals(links, abi.MAX_HELD_FRAMES))
    return out


def check_rows(t, h, pr, seed, params, genes, b, stats, name, want_hits):
    """bioik_eval_check on a few rows under two sets of thresholds; in every other row the Position / Orientation / Pose goals get the row's own R as their target"""
    n = genes.shape[0]
    hits = 0
    rows = list(range(0, n, max(n // 16, 1)))
    for sp in (abi.default_solve_params(dpos=-1.0, drot=-1.0, dtwist=1e-3), abi.default_solve_params(dpos=1e-3, drot=0.5, dtwist=-1.0)):
        for j, i in enumerate(rows):
            fr, Rp = exact_frames(pr, seed, genes[i:i + 1])
            dp, dq = {l: b.dp(l)[i:i + 1] for l in b.m}, {l: b.dq(l)[i:i + 1] for l in b.m}
            P1 = params.copy()
            if j % 2 == 0:
                for g, off in zip(t.goals, t.param_offsets):
                    p, q, _, _ = goal_frame(t, g, fr, dp, dq)
                    if g.opcode in (abi.GOAL_POSITION, abi.GOAL_POSE):
                        P1[off:off + 3] = np.asarray(p[0], dtype=np.float64)
                    if g.opcode in (abi.GOAL_ORIENTATION, abi.GOAL_POSE):
                        o = off + (3 if g.opcode == abi.GOAL_POSE else 0)
                        P1[o:o + 4] = np.asarray(q[0], dtype=np.float64)
            ok, band, _ = success_test(t, pr, P1, Rp, *rr.thresholds(sp), dp, dq)
            got = bool(h.check(sp, seed, P1, genes[i:i + 1])[0])
            stats.rows += 1
            stats.band += int(band[0])
            assert got == bool(ok[0]) or band[0], "%s: the success test differs outside the band at row %d (device %s, long double %s)" % (name, i, got, ok[0])
            hits += int(got)
    if want_hits:
        assert 0 < hits < 2 * len(rows), (name, hits)


def function_level(make_solver, name, stats, n=200):
    """bioik_eval_fitness in both FK modes, bioik_eval_check and bioik_eval_fk against the restatement; the worst error / bound ratios go to `stats`"""
    model, group, goals = function_cases()[name]
    t = ProblemTemplate(model, group, goals)
    h = make_solver(t)
    for g in goals:  # the base link is a tip of the problem like the goal's own link
        assert model.link_index(g.link_name()) in h.tip_links and (base_of(g) is None or model.link_index(base_of(g)) in h.tip_links), name
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    rng = np.random.default_rng(sum(map(ord, name)))
    lo, hi = np.asarray(model.var_min), np.asarray(model.var_max)
    seed = lo + (hi - lo) * rng.random(model.n_variables)
    X = lo + (hi - lo) * rng.random((n, model.n_variables))
    genes = np.ascontiguousarray(X[:, pr.active])
    params = t.pack_params()
    b = rr.Bounds(pr, pr.full(seed, genes).astype(np.float64))
    fr, _ = exact_frames(pr, seed, genes)
    dp, dq = {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}
    # bioik_eval_fk: the base link's frame is among the tips
    tips = h.fk_genes(seed, genes)
    for i, l in enumerate(h.tip_links):
        assert stats.ratio("fk position", np.linalg.norm(tips[:, i, :3] - np.asarray(fr[int(l)][0], dtype=np.float64), axis=1), dp[int(l)], name) <= 1.0, (name, l)
    cost, bound = costs_and_bounds(t, params, fr, dp, dq)
    want, bnd = total(cost, bound)
    got, sec = h.fitness(abi.FK_EXACT, seed, params, genes)
    err = np.abs(got - want)
    r = stats.ratio("exact primary", err, np.maximum(bnd, 1e-300), name)
    assert r <= 1.0, "%s: exact fitness off by %.3g, bound %.3g (row %d)" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))], int(np.argmax(err / np.maximum(bnd, 1e-300))))
    assert not sec.any(), name
    check_rows(t, h, pr, seed, params, genes, b, stats, name, all(g.opcode in FRAME_GOALS for g in goals))
    # linearised phenotypes around a base: frames and their bounds as touch_cases.function_level builds them; R from the unnormalised quaternions as they are
    base = genes[0]
    near = np.ascontiguousarray(base + 0.02 * rng.normal(size=(max(n // 8, 4), len(pr.active))))
    tb_l, dl_l = pr.approximator(seed, base)
    lf = pr.linear_frames(tb_l, dl_l, base, near)
    bi = rr.Bounds(pr, pr.full(seed, base[None]).astype(np.float64))
    bl = rr.Bounds(pr, pr.full(seed, near).astype(np.float64))
    dv = np.abs(near - base[None])
    dpl, dql = {}, {}
    for ti, tl in enumerate(pr.tips):
        tabs = np.full(len(pr.active), 2 * bl.dq(tl)[0] * (bl.lam[tl][0] + 1) * 4)
        mag = np.abs(np.asarray(dl_l[ti], dtype=np.float64)).max(axis=1)
        dpl[tl] = bi.dp(tl)[0] + dv @ tabs + C * U * (dv @ mag)
        dql[tl] = bi.dq(tl)[0] + dv @ tabs + C * U * (dv @ mag)
    cost, bound = costs_and_bounds(t, params, lf, dpl, dql)
    want, bnd = total(cost, bound)
    pl, _ = h.fitness(abi.FK_LINEAR, seed, params, near, base)
    err = np.abs(pl - want)
    r = stats.ratio("linear primary", err, np.maximum(bnd, 1e-300), name)
    assert r <= 1.0, "%s: linearised fitness off by %.3g, bound %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))])
    h.close()


def streamed(make_solver, device_arrays):
    """bioik_stream_fitness_device (genes [unit][D][pop]) gives the bits of bioik_eval_fitness, exact FK, on the same library"""
    model, group, goals = function_cases()["two_bases_one_link"]
    t = ProblemTemplate(model, group, goals)
    h = make_solver(t)
    rng = np.random.default_rng(3)
    units, pop = 2, 77
    lo, hi = np.asarray(model.var_min), np.asarray(model.var_max)
    seeds = np.ascontiguousarray(lo + (hi - lo) * rng.random((units, model.n_variables)))
    params = np.ascontiguousarray(np.tile(t.pack_params(), (units, 1)))
    genes = np.ascontiguousarray(rng.uniform(-1, 1, size=(units, h.D, pop)))
    (ds, _), (dp_, _), (dg, _), (df, fetch) = (device_arrays(a) for a in (seeds, params, genes, np.zeros((units, pop))))
    h.stream_fitness_device(units, pop, ds, dp_, dg, df, 0)
    got = fetch()
    for u in range(units):
        want, _ = h.fitness(abi.FK_EXACT, seeds[u], params[u], np.ascontiguousarray(genes[u].T))
        assert np.array_equal(got[u], want), u
    h.close()


# ---- identity and refusals ----------------------------------------------------------------------------------------------------------------------------------
class ExplicitWorld(ProblemTemplate):
    """a template that passes goal_base_link as an array of -1 where ProblemTemplate passes NULL"""

    def desc(self):
        d = super().desc()
        d.goal_base_link = abi.iptr(self._goal_base_link)
        return d


class RawBase(ProblemTemplate):
    """a template whose goal_base_link is what the test writes (link indices no name stands for)"""

    def __init__(self, model, group, goals, raw):
        super().__init__(model, group, goals)
        self._goal_base_link[:len(raw)] = raw

    def desc(self):
        d = super().desc()
        d.goal_base_link = abi.iptr(self._goal_base_link)
        return d


def identity(make_solver, report):
    """goal_base_link all -1 and goal_base_link NULL: the same launches, kernels and bits on the arm (whose kernels are the lean ones)"""
    from bio_ik_amd.workload import make_queries
    goals = [PoseGoal(RW)]
    res, launches = [], []
    for cls in (ProblemTemplate, ExplicitWorld):
        t = cls(pr2_like(), "right_arm", goals)
        assert (t.desc().goal_base_link is None or not t.desc().goal_base_link) == (cls is ProblemTemplate)
        h = make_solver(t)
        seeds, params, _ = make_queries(t, h.active_variables, h.fk_genes, 16, seed=9)
        report.read()
        res.append(h.solve_batch(abi.default_solve_params(population=128, max_steps=16, islands=2, random_seed=3), seeds, params))
        launches.append(report.kernels(report.read()))
        h.close()
    assert launches[0] == launches[1] and launches[0] and all(k.startswith("k_solve_lean") or k.startswith("k_select") for k in launches[0]), launches
    assert all(np.array_equal(a, b) for a, b in zip(*res))


def refusals(make_solver, lib):
    """every row of the table of include/bioik_hip.h (BASE LINKS), with its status code; bioik_last_error() names the goal; outputs stay untouched"""
    m = pr2_like()
    sec = PositionGoal(LW, base_link=RW)
    sec.secondary_ = True
    box = pr2_like()
    box.add_collision_box(LW, (0.1, 0.06, 0.04))
    tree, links = held_limit_model()
    rows = [
        (RawBase(m, "all", [PositionGoal(RW), PositionGoal(LW)], [-1, m.n_links]), abi.ERR_NOT_FOUND, "goal 1"),
        (RawBase(m, "all", [PositionGoal(RW), PositionGoal(LW)], [m.link_index(RW), -1]), abi.ERR_INVALID_ARGUMENT, "goal 0"),  # its own link
        (ProblemTemplate(m, "all", [PositionGoal(RW), sec]), abi.ERR_UNSUPPORTED, "goal 1"),
        (ProblemTemplate(box, "all", [PositionGoal(RW), TouchGoal(LW, (0, 0, 0), (0, 0, 1), base_link=RW)]), abi.ERR_UNSUPPORTED, "goal 1"),
        (ProblemTemplate(tree, "g", held_limit_goals(links, abi.MAX_HELD_FRAMES + 1)), abi.ERR_UNSUPPORTED, "goal %d" % abi.MAX_HELD_FRAMES),
    ]
    from bio_ik_amd import BalanceGoal, JointVariableGoal
    massive = pr2_like()
    massive.link_mass[massive.link_index(RW)] = 1.0
    rows.append((RawBase(massive, "all", [PositionGoal(RW), BalanceGoal((0, 0, 0))], [-1, massive.link_index(LW)]), abi.ERR_INVALID_ARGUMENT, "goal 1"))  # (names no link)
    rows.append((RawBase(m, "all", [PositionGoal(RW), JointVariableGoal("r_elbow_flex_joint", -1.0)], [-1, m.link_index(LW)]), abi.ERR_INVALID_ARGUMENT, "goal 1"))
    for t, code, word in rows:
        try:
            make_solver(t)
        except solver.BioIKError as e:
            assert e.code == code and word in str(e) and word in lib.bioik_last_error().decode(), (code, word, e.code, str(e))
        else:
            raise AssertionError("accepted: %s %s" % (code, word))
    # BIOIK_MODE_JAC on a problem with a based goal: refused by the solve call, nothing launched, the outputs keep their pattern; gd on the same arrays works
    t = ProblemTemplate(m, "all", [PoseGoal(RW), PoseGoal(LW, base_link=RW)])
    h = make_solver(t)
    n = 3
    seeds = np.tile(np.asarray(m.default_positions(), dtype=np.float64), (n, 1))
    params = np.tile(t.pack_params(), (n, 1))
    sol, fit = np.full((n, h.V), 7.25), np.full(n, 7.25)
    suc, steps = np.full(n, 77, dtype=np.int32), np.full(n, 77, dtype=np.int32)
    p = abi.default_solve_params(mode="jac", max_steps=4, islands=1)
    rc = lib.bioik_solve_batch(h.problem, p, n, solver._d(seeds), solver._d(params), solver._d(sol), solver._d(fit), solver._i(suc), solver._i(steps))
    assert rc == abi.ERR_UNSUPPORTED and "JAC" in lib.bioik_last_error().decode(), (rc, lib.bioik_last_error())
    assert (sol == 7.25).all() and (fit == 7.25).all() and (suc == 77).all() and (steps == 77).all()
    for mode in ("gd", "gd_c"):
        h.solve_batch(abi.default_solve_params(mode=mode, max_steps=2, islands=1), seeds, params)
    h.close()


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------------------------
N_QUERIES = 16
SOLVE = dict(population=128, max_steps=64, islands=4, random_seed=5)  # (dtwist: the default, 1e-5)
AXIS = (1.0, 0.0, 0.0)


def solve_template(variant):
    if variant == "tray":  # the left wrist keeps a pose in the right wrist's frame while the right wrist is posed in the world
        return ProblemTemplate(pr2_like(), "all", [PoseGoal(RW), PoseGoal(LW, base_link=RW)])
    if variant == "apart":  # both wrists placed, and at least a distance apart
        return ProblemTemplate(pr2_like(), "all", [PositionGoal(RW), PositionGoal(LW), MinDistanceGoal(LW, (0, 0, 0), 0.1, base_link=RW)])
    assert variant == "aim"  # the left wrist's x axis points at a spot given in the right wrist's frame
    return ProblemTemplate(pr2_like(), "all", [LookAtGoal(LW, AXIS, (0, 0, 0), base_link=RW)])


def reachable_queries(t, h, n=N_QUERIES, seed=11, start=0.4):
    """per query a random configuration inside the limits; every goal's numbers from its long-double FK (R for a based goal), so that the configuration meets
    all of them; the solve starts from a configuration whose active variables lie up to `start` (rad, m) from it, clipped to the limits -- inside the
    +-0.5 windows of the bounded variant.  (From a start drawn over the whole range the 15-variable "tray" problem stayed near the floor within 64 steps: 9 of
    16 under exact FK, 6 under linearised phenotypes, measured on the host simulator.)"""
    m = t.model
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    target = lo + (hi - lo) * rng.random((n, m.n_variables))
    seeds = np.clip(target + start * rng.uniform(-1.0, 1.0, size=target.shape), lo, hi)
    seeds = np.ascontiguousarray(np.where(np.isin(np.arange(m.n_variables), pr.active)[None], seeds, target))
    fr, _ = exact_frames(pr, target[0], target[:, pr.active])
    zero = {l: np.zeros(n) for l in fr}
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        p, q, _, _ = goal_frame(t, g, fr, zero, zero)
        p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
        if g.opcode == abi.GOAL_POSITION:
            params[:, off:off + 3] = p
        elif g.opcode == abi.GOAL_POSE:
            params[:, off:off + 3], params[:, off + 3:off + 7], params[:, off + 7] = p, q, 0.5
        elif g.opcode == abi.GOAL_MIN_DISTANCE:  # the base's origin, nine tenths of the distance the configuration has
            params[:, off + 3] = 0.9 * np.linalg.norm(p, axis=1)
        elif g.opcode == abi.GOAL_LOOK_AT:  # a spot 0.3 m along the axis as the configuration has it
            params[:, off:off + 3] = AXIS
            params[:, off + 3:off + 6] = p + 0.3 * np.asarray(np_goals.qrot(np.asarray(q, dtype=LD), AXIS), dtype=np.float64)
        else:
            raise AssertionError(g.opcode)
    return seeds, params


def verify_solve(t, h, seeds, params, sol, fit, suc, min_success, sp):
    """every row flagged a success passes the long-double success test on R recomputed from the returned solution, with the bound as slack; the fitness is the
    long-double cost within its bound; inactive variables are the seed's.  Returns the number of successes."""
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    inactive = np.setdiff1d(np.arange(h.V), pr.active)
    won = 0
    for i in range(sol.shape[0]):
        g1 = sol[i:i + 1, pr.active]
        b = rr.Bounds(pr, sol[i:i + 1].astype(np.float64))
        dp, dq = {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}
        fr, Rp = exact_frames(pr, sol[i], g1)
        assert np.array_equal(sol[i, inactive], seeds[i, inactive])
        if suc[i]:
            _, _, margins = success_test(t, pr, params[i], Rp, *rr.thresholds(sp), dp, dq)
            for v, bnd in margins:
                assert v[0] <= bnd[0], (i, v[0], bnd[0])
        cost, bound = costs_and_bounds(t, params[i], fr, dp, dq)
        want, bnd = total(cost, bound)
        assert abs(fit[i] - want[0]) <= bnd[0], (i, fit[i], want[0], bnd[0])
        won += int(suc[i])
    assert won >= min_success, "%d of %d queries solved" % (won, sol.shape[0])
    return won


GRADIENT_KINDS = ("gd", "gd_r", "gd_c")
TRAY_KINDS = ["gd_r", "gd", "gd_c", "ranked", "bounded", "migration", "island_sync", "timeout"]
GD_START, GD_DTWIST = 0.03, 2e-2


def sharded(make, kind, p, seeds, params, bounds, workers):
    """the call solved by `workers` handles on as many host threads, each a slice of the queries announced by its global offset (bioik_problem_set_first_query: a
    query's answer is a function of its global index, not of the call it comes in): the rows of the one call, sooner -- the host simulator steps every lane of a
    solve on the thread that calls it"""
    import threading
    n = seeds.shape[0]
    cuts = [n * w // workers for w in range(workers + 1)]
    handles = [make() for _ in range(workers)]
    solver.sync_debug_switches(handles[0].L)  # (once, before any thread solves)
    out, errors = [None] * workers, []

    def work(w):
        try:
            a, b = cuts[w], cuts[w + 1]
            if a == b:
                return
            handles[w].set_first_query(a)
            bw = None if bounds is None else (bounds[0][a:b], bounds[1][a:b])
            out[w] = handles[w].solve_batch_ranked(p, seeds[a:b], params[a:b], 2, 0.0) if kind == "ranked" else handles[w].solve_batch(p, seeds[a:b], params[a:b], bounds=bw)
        except Exception as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(w,)) for w in range(workers)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for hw in handles:
        hw.close()
    assert not errors, errors
    parts = [o for o in out if o is not None]
    return tuple(np.concatenate([part[i] for part in parts]) for i in range(len(parts[0])))


def whole_solve(make_solver, variant, kind="plain", fk=abi.FK_EXACT, workers=1):
    """variant: tray | apart | aim; kind: plain | gd | gd_r | gd_c | ranked (k = 2) | bounded (+-0.5 around the seed) | migration (E = 2) | island_sync | timeout (a
    generous one: the device-clock path, the bits of the call without).  workers > 1: the call in slices on as many threads (`sharded`).  Returns (solver,
    template, seeds, params, solve parameters, bounds, results) for bit comparisons."""
    t = solve_template(variant)
    h = make_solver(t)
    # The gradient family converges linearly: on "tray" 64 steps of gd / gd_r take the fitness down by a factor of about 27 wherever they start, gd_c by about
    # 3e4 (measured on the host simulator from starts 0.1 ... 1e-4 away), and the default success test asks for a cost near 1e-10.  So these variants -- and only
    # these -- start GD_START from their targets and are judged with dtwist = GD_DTWIST: a descent of 64 real steps that a part of the queries completes.
    seeds, params = reachable_queries(t, h, start=GD_START if kind in GRADIENT_KINDS else 0.4)
    p = abi.default_solve_params(fk_mode=fk, **SOLVE)
    bounds = None
    floor = N_QUERIES // 2
    if kind in GRADIENT_KINDS:
        p = abi.default_solve_params(mode=kind, max_steps=64, islands=4, random_seed=5, dtwist=GD_DTWIST)
        floor = N_QUERIES // 2 if kind == "gd_r" else 0  # (the issue sets the floor for gd_r; gd and gd_c: the fitness against its bound, the bits against the simulator)
    if kind == "migration":
        p.island_migration = 2
    if kind == "island_sync":
        p.island_sync = 1
    if kind == "timeout":
        p.timeout = 3600.0
    solve = (lambda pp: sharded(lambda: make_solver(t), kind, pp, seeds, params, bounds, workers)) if workers > 1 else (lambda pp: h.solve_batch(pp, seeds, params, bounds=bounds))
    if kind == "bounded":
        bounds = (seeds - 0.5, seeds + 0.5)
    if kind == "ranked":
        sol, fit, suc, steps, count = sharded(lambda: make_solver(t), kind, p, seeds, params, None, workers) if workers > 1 else h.solve_batch_ranked(p, seeds, params, 2, 0.0)
        assert count.min() >= 1
        best = sharded(lambda: make_solver(t), "plain", p, seeds, params, None, workers) if workers > 1 else h.solve_batch(p, seeds, params)
        assert all(np.array_equal(a[:, 0], b) for a, b in zip((sol, fit, suc, steps), best))  # row 0: the plain answer
        for r in range(2):
            rows = count > r
            verify_solve(t, h, seeds[rows], params[rows], sol[rows, r], fit[rows, r], suc[rows, r], floor if r == 0 else 0, p)
        res = (sol, fit, suc, steps, count)
    else:
        res = solve(p)
        won = verify_solve(t, h, seeds, params, res[0], res[1], res[2], floor, p)
        print("\n[base links] %s %s fk %d: %d of %d solved, steps %d ... %d" % (variant, kind, fk, won, len(seeds), res[3].min(), res[3].max()))
        if kind == "timeout":  # an hour is never reached: the answer of the call without a timeout, through the kernels' deadline path
            q = abi.default_solve_params(fk_mode=fk, **SOLVE)
            assert all(np.array_equal(a, b) for a, b in zip(res, solve(q)))
        if kind == "island_sync":  # every island of a query stops at the end of the first step in which one passes: a solved query's steps are at most the plain call's
            plain = solve(abi.default_solve_params(fk_mode=fk, **SOLVE))
            both = (res[2] == 1) & (plain[2] == 1)
            assert both.any() and (res[3][both] <= plain[3][both]).all(), (res[3], plain[3])
        if bounds is not None:
            act = np.asarray(h.active_variables)
            assert (res[0][:, act] >= bounds[0][:, act]).all() and (res[0][:, act] <= bounds[1][:, act]).all()
    return h, t, seeds, params, p, bounds, res


def simulator_answer(make_sim, kind, p, seeds, params, bounds, workers=8):
    """all rows of the call on the host simulator (make_sim(): a handle of the problem on the simulator), in slices on `workers` threads"""
    return sharded(make_sim, kind, p, seeds, params, bounds, workers)


def mapping_independence(make_solver, monkeypatch, report, variants=("tray", "aim"), steps=SOLVE["max_steps"], n=N_QUERIES, islands=SOLVE["islands"]):
    """the whole-solve cases give the same bits under every lane mapping the BIOIK_SOLVE_* switches can force, and the report names only the general flavour's
    kernels (k_solve, k_solve_bounded, k_solve_point*) and the islands' selection for these problems"""
    for variant in variants:
        t = solve_template(variant)
        h = make_solver(t)
        seeds, params = reachable_queries(t, h, n)
        for fk in (abi.FK_EXACT, abi.FK_LINEAR):
            p = abi.default_solve_params(population=128, max_steps=steps, islands=islands, random_seed=5, fk_mode=fk)
            report.read()
            base = h.solve_batch(p, seeds, params)
            for env in tc.MAPPINGS:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                got = h.solve_batch(p, seeds, params)
                for k in env:
                    monkeypatch.delenv(k)
                assert all(np.array_equal(a, b) for a, b in zip(base, got)), (variant, fk, env)
            kernels = set(report.kernels(report.read()))
            assert kernels and kernels <= {"k_solve", "k_solve_bounded", "k_solve_point", "k_solve_point_bounded", "k_select", "k_select_wave"}, kernels
        h.close()
