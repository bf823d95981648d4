"""SelfClearanceGoal (opcode 20) on the library under test: the GPU suite (tests/test_gpu_self_clearance.py) and the host simulator
(tests/test_hostsim_self_clearance.py) run these cases.  `make_solver(template)` makes a bio_ik_amd.solver.HipSolver of the library under test.

The pin is the goal restated in long double from its definition (include/bioik_hip.h: BIOIK_GOAL_SELF_CLEARANCE) out of two pieces that exist and are imported as they
are: with A the other link's frame and B the goal link's frame (long-double forward kinematics of tests/np_fk.py),

    R, (dR.p, dR.q) = base_link_cases.relative(A, B), base_link_cases.relative_bound(A, B, FK bounds of both tips)
    cost, bound     = clearance_cases.clearance(margin, R.p, R.q, points of the link, points of the other link, dR.p, dR.q)

and weight^2 on both (plus C U |cost| for that product), as clearance_cases.costs_and_bounds does for opcode 19.  Not the oracle (it does not know the opcode) and not
the kernel.  The check is error <= bound; -s prints the worst ratios."""
import ctypes
import functools
import types

import numpy as np

import base_link_cases as bl
import clearance_cases as cc
import np_goals
import random_robot_cases as rr
import touch_cases as tc
from bio_ik_amd import ClearanceGoal, PoseGoal, PositionGoal, ProblemTemplate, SelfClearanceGoal, TouchGoal, abi, pr2_like, solver
from np_fk import LD

C, U = rr.C, rr.U
RW, LW, RE, LE = bl.RW, bl.LW, bl.RE, bl.LE
RF, LF = "r_forearm_link", "l_forearm_link"
SELF = abi.GOAL_SELF_CLEARANCE
POINT_COUNTS, OTHER_COUNTS = (1, 2, 3, 17), (1, 2, 3, 9, abi.MAX_OBSTACLES)


# ---- models -------------------------------------------------------------------------------------------------------------------------------------------------
def balls(m, seed, rmin, rmax, scale=0.08):
    rng = np.random.default_rng(500 + seed)
    return rng.uniform(-scale, scale, size=(m, 3)), rng.uniform(rmin, rmax, size=m)


def with_points(model, *tables):
    """model with (link, centres, radii) tables added"""
    for link, pts, rad in tables:
        model.add_collision_points(link, pts, rad)
    return model


def pair_model(n, m, seed=1, link=RW, other=LW, model=None, rmin=0.15, rmax=0.35):
    """n small spheres on `link`, m large ones on `other`: two wrists of a random population are often nearer than 0.4 m, so some pair penetrates"""
    return with_points(model or pr2_like(), (link, *cc.spheres(n, seed)), (other, *balls(m, seed, rmin, rmax)))


def function_cases():
    """name -> (model, group, goals): the trip counts of both loops (odd, even, the leftover trip, the cap, the first and the last trip of the load-ahead), both states
    of the held-is-own bit, the places a based row can sit, the tables' places in the buffer"""
    out = {}
    for n in POINT_COUNTS:
        for m in OTHER_COUNTS:
            out["points_%d_other_%d" % (n, m)] = (pair_model(n, m, 7 * n + m), "all", [SelfClearanceGoal(RW, LW, 0.01)])
    u4 = (0.1, 0.2, 0.3, 0.9)
    # the other link completed before the goal's link, and after it (the walk completes the tips in the order their links are first named)
    out["other_first"] = (pair_model(3, 4), "all", [PositionGoal(LW, (0.5, 0.2, 0.8)), SelfClearanceGoal(RW, LW, 0.01)])
    out["other_last"] = (pair_model(3, 4), "all", [PositionGoal(RW, (0.6, -0.2, 0.8)), SelfClearanceGoal(RW, LW, 0.01)])
    # two links of one chain, either way round
    out["elbow_against_wrist"] = (pair_model(3, 4, 2, RW, RE), "right_arm", [SelfClearanceGoal(RW, RE, 0.01)])
    out["wrist_against_elbow"] = (pair_model(3, 4, 3, RE, RW), "right_arm", [SelfClearanceGoal(RE, RW, 0.01)])
    # the other link on the root; behind a fixed trailing frame (both links)
    out["other_is_root"] = (pair_model(3, 4, 4, RW, "base_link", rmin=0.3, rmax=0.6), "right_arm", [SelfClearanceGoal(RW, "base_link", 0.01)])
    out["other_has_trailing_frame"] = (pair_model(3, 4, 5, "l_tool", "r_tool", model=bl.tool_model()), "all", [SelfClearanceGoal("l_tool", "r_tool", 0.01)])
    # two goals sharing one held link; two goals on one tip
    m = with_points(pair_model(3, 4, 6, LW, RW), (LE, *cc.spheres(2, 9)))
    out["two_goals_one_held_link"] = (m, "all", [SelfClearanceGoal(LW, RW, 0.01), SelfClearanceGoal(LE, RW, 0.02, weight=0.7)])
    m = with_points(pair_model(3, 4, 7, LW, RW), (RE, *balls(5, 8, 0.1, 0.3)))
    out["two_goals_one_tip"] = (m, "all", [PositionGoal(RW, (0.6, -0.2, 0.8)), PositionGoal(RE, (0.4, -0.2, 0.9), weight=0.3), SelfClearanceGoal(LW, RW, 0.01),
                                          SelfClearanceGoal(LW, RE, 0.0, weight=0.8)])
    # beside a PoseGoal on the same tip (the tip's one-PoseGoal form must not be taken); as its tip's only goal; as the problem's only goal
    out["beside_pose_goal"] = (pair_model(3, 4, 8, LW, RW), "all", [PoseGoal(RW, (0.6, -0.2, 0.8), u4), PoseGoal(LW, (0.5, 0.3, 0.9), u4, weight=0.6), SelfClearanceGoal(LW, RW, 0.01)])
    out["only_goal_of_its_tip"] = (pair_model(3, 4, 9, LW, RW), "all", [PoseGoal(RW, (0.6, -0.2, 0.8), u4), SelfClearanceGoal(LW, RW, 0.01)])
    out["only_goal"] = (pair_model(3, 4, 10, LW, RW), "all", [SelfClearanceGoal(LW, RW, 0.01)])
    # beside a world ClearanceGoal that reads the same link's points; behind a TouchGoal's rows in the buffer
    out["beside_world_clearance"] = (pair_model(3, 4, 11, LW, RW), "all", [ClearanceGoal(LW, 0.01, cc.scene(9, 3, box=((0.2, -0.3, 0.4), (0.9, 0.7, 1.3))), weight=1.3), SelfClearanceGoal(LW, RW, 0.02)])
    out["behind_touch"] = (pair_model(3, 4, 12, LW, RW), "all", [TouchGoal(RW, (0.55, -0.2, 0.7), (0.2, -0.3, 0.9), weight=0.7), SelfClearanceGoal(LW, RW, 0.01, weight=0.6)])
    out["weight"] = (pair_model(3, 4, 13), "all", [SelfClearanceGoal(RW, LW, 0.01, weight=0.37)])
    # exact zeros: s <= 0 for every pair; every pair far apart (the other link's spheres 100 m off in its own frame)
    out["negative_margin"] = (pair_model(3, 9, 14, rmin=5.0, rmax=6.0), "all", [SelfClearanceGoal(RW, LW, -20.0)])
    far = balls(9, 15, 0.15, 0.35)
    out["all_far"] = (with_points(pr2_like(), (RW, *cc.spheres(3, 15)), (LW, far[0] + np.array([100.0, 0, 0]), far[1])), "all", [SelfClearanceGoal(RW, LW, 0.02)])
    out["all_penetrating"] = (pair_model(3, 9, 16, rmin=5.0, rmax=6.0), "all", [SelfClearanceGoal(RW, LW, 0.02)])
    # one ball around the left wrist that a part of a random population's right wrists is inside of (chosen on the CPU: the restatement counts 5 % ... 95 % of the rows)
    out["some_individuals"] = (with_points(pr2_like(), (RW, *cc.spheres(3, 17)), (LW, [[0.0, 0.0, 0.0]], [0.55])), "all", [SelfClearanceGoal(RW, LW, 0.0)])
    return out


# ---- costs and bounds ---------------------------------------------------------------------------------------------------------------------------------------
def costs_and_bounds(t, tables, params, frames, dp, dq, depth=None):
    """weighted cost (n, n_goals) in long double and its bound, for frames {link: (p, q)} known to dp / dq {link: (n,)}; the goals that are no SelfClearanceGoal:
    clearance_cases.costs_and_bounds (`tables`: {goal index: rows} of the ClearanceGoals).  `depth` (optional dict): per SelfClearanceGoal its deepest penetration"""
    n = next(iter(frames.values()))[0].shape[0]
    cost = np.zeros((n, len(t.goals)), dtype=LD)
    bound = np.zeros((n, len(t.goals)))
    others = [k for k, g in enumerate(t.goals) if g.opcode != SELF]
    if others:
        shim = types.SimpleNamespace(goals=[t.goals[k] for k in others], param_offsets=[t.param_offsets[k] for k in others], model=t.model)
        c, b = cc.costs_and_bounds(shim, {i: tables[k] for i, k in enumerate(others) if k in tables}, params, frames, dp, dq)
        cost[:, others], bound[:, others] = c, b
    for k, (g, off) in enumerate(zip(t.goals, t.param_offsets)):
        if g.opcode != SELF:
            continue
        link, other = t.model.link_index(g.link_name()), t.model.link_index(g.getOtherLinkName())
        (pB, qB), (pA, qA) = frames[link], frames[other]
        bc = lambda a: np.broadcast_to(a, (n,))  # noqa: E731
        p, q = bl.relative(pA, qA, pB, qB)
        d_p, d_q = bl.relative_bound(pA, qA, pB, qB, bc(dp[other]), bc(dq[other]), bc(dp[link]), bc(dq[link]))
        c, b, deep = cc.clearance(params[off], p, q, t.model.collision_points(link), t.model.collision_points(other), d_p, d_q)
        w2 = LD(g.getWeight()) ** 2
        cost[:, k] = c * w2
        bound[:, k] = float(w2) * b + C * U * np.abs(np.asarray(cost[:, k], dtype=np.float64))
        if depth is not None:
            depth[k] = deep
    return cost, bound


def least_gap(t, g, frames, i):
    """min_ij |w_i - c_j| - r_i - R_j of row i, long double"""
    link, other = t.model.link_index(g.link_name()), t.model.link_index(g.getOtherLinkName())
    p, q = bl.relative(frames[other][0][i:i + 1], frames[other][1][i:i + 1], frames[link][0][i:i + 1], frames[link][1][i:i + 1])
    pts = np.asarray(t.model.collision_points(link), dtype=LD).reshape(-1, 4)
    obs = np.asarray(t.model.collision_points(other), dtype=LD).reshape(-1, 4)
    w = cc.world_points(p, q, pts)[0]
    return float((np.sqrt(((w[:, None, :] - obs[None, :, :3]) ** 2).sum(axis=2)) - pts[:, 3:4] - obs[None, :, 3]).min())


def linear_bounds(pr, seed, base, near, dl_l):
    """FK bounds of linearised phenotypes, as clearance_cases.function_level builds them"""
    bi = rr.Bounds(pr, pr.full(seed, base[None]).astype(np.float64))
    bnear = rr.Bounds(pr, pr.full(seed, near).astype(np.float64))
    dv = np.abs(near - base[None])
    dp, dq = {}, {}
    for ti, tl in enumerate(pr.tips):
        tabs = np.full(len(pr.active), 2 * bnear.dq(tl)[0] * (bnear.lam[tl][0] + 1) * 4)
        mag = np.abs(np.asarray(dl_l[ti], dtype=np.float64)).max(axis=1)
        dp[tl] = bi.dp(tl)[0] + dv @ tabs + C * U * (dv @ mag)
        dq[tl] = bi.dq(tl)[0] + dv @ tabs + C * U * (dv @ mag)
    return dp, dq


def setup(make_solver, model, group, goals, name, n):
    t = ProblemTemplate(model, group, goals)
    h = make_solver(t)
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    seed, genes = cc.population(model, pr, np.random.default_rng(sum(map(ord, name))), n)
    return t, h, pr, seed, genes


def exact_against(t, h, pr, seed, params, genes, stats, name):
    b = rr.Bounds(pr, pr.full(seed, genes).astype(np.float64))
    fr = tc.exact_frames(pr, seed, genes)
    cost, bound = costs_and_bounds(t, t.obstacle_tables(), params, fr, {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m})
    pa, sa = h.fitness(abi.FK_EXACT, seed, params, genes)
    want, bnd = tc.sums(t, cost, bound)[0]
    err = np.abs(pa - want)
    r = stats.ratio("exact primary", err, np.maximum(bnd, 1e-300), name)
    worst = int(np.argmax(err / np.maximum(bnd, 1e-300)))
    assert r <= 1.0, "%s: exact primary fitness off by %.3g, bound %.3g (row %d)" % (name, err.max(), bnd[worst], worst)
    assert not sa.any(), name
    return pa, cost, bound, b, fr


def function_level(make_solver, name, stats, n=200):
    """bioik_eval_fitness in both FK modes and bioik_eval_check against the restatement; the worst error / bound ratios go to `stats`.  Returns the exact primary fitness."""
    model, group, goals = function_cases()[name]
    t, h, pr, seed, genes = setup(make_solver, model, group, goals, name, n)
    for g in goals:
        if g.opcode == SELF:  # both links are tips of the problem
            assert model.link_index(g.link_name()) in h.tip_links and model.link_index(g.getOtherLinkName()) in h.tip_links, name
    params = t.pack_params()
    pa, cost, _, b, fr = exact_against(t, h, pr, seed, params, genes, stats, name)
    own = [k for k, g in enumerate(t.goals) if g.opcode == SELF]
    own64 = np.asarray(cost[:, own], dtype=np.float64)
    if name in ("all_far", "negative_margin"):
        assert np.all(pa == 0.0) and np.all(own64 == 0.0), name  # exactly nothing, not "small"
    if name.startswith("points_"):
        assert np.any(pa > 0.0) and not np.all(pa > 0.0), name  # (every case of the grid takes the branch somewhere, and leaves it somewhere)
    if name == "all_penetrating":
        depth = {}
        costs_and_bounds(t, {}, params, fr, {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, depth)
        assert np.all(depth[0] > 1.0) and np.all(pa > 0.0), name
    if name == "some_individuals":
        for hit in (int(np.count_nonzero(own64[:, 0] > 0.0)), int(np.count_nonzero(pa > 0.0))):  # the restatement alone, then the library
            assert n // 20 < hit < n - n // 20, (name, hit)
    # the success test (the default branch): weighted cost < min(dpos, dtwist)^2 for every primary goal.  Per row the margin of every SelfClearanceGoal is set from the
    # row's own least gap: 1 mm below it nothing penetrates and the cost is 0, provably a success; 1 cm / weight above it some pair penetrates by that much and the
    # weighted cost is at least 1e-4 > 1e-6, provably none (clearance_cases.function_level)
    if len(own) == len(t.goals):
        sp = abi.default_solve_params(dpos=-1.0, drot=-1.0, dtwist=1e-3)
        rows = list(range(0, n, max(n // 16, 1)))
        hits = 0
        for j, i in enumerate(rows):
            P1 = params.copy()
            for k in own:
                P1[t.param_offsets[k]] = least_gap(t, t.goals[k], fr, i) + (-1e-3 if j % 2 == 0 else 1e-2 / abs(t.goals[k].getWeight()))
            f1 = {l: (fr[l][0][i:i + 1], fr[l][1][i:i + 1]) for l in fr}
            c1, b1 = costs_and_bounds(t, {}, P1, f1, {l: b.dp(l)[i:i + 1] for l in b.m}, {l: b.dq(l)[i:i + 1] for l in b.m})
            ok = int(h.check(sp, seed, P1, genes[i:i + 1])[0])
            sure_yes = all(float(c1[0, k]) + b1[0, k] < 1e-6 for k in own)
            sure_no = any(float(c1[0, k]) - b1[0, k] >= 1e-6 for k in own)
            assert sure_yes == (j % 2 == 0) and sure_no == (j % 2 == 1), (name, i, [float(c1[0, k]) for k in own])
            assert ok == (1 if sure_yes else 0), (name, i, ok, [float(c1[0, k]) for k in own])
            hits += ok
        assert hits == (len(rows) + 1) // 2, (name, hits)
    # linearised phenotypes around a base: R from the unnormalised quaternions as they are
    rng = np.random.default_rng(len(name))
    base = genes[0]
    near = np.ascontiguousarray(base + 0.02 * rng.normal(size=(max(n // 8, 4), len(pr.active))))
    tb_l, dl_l = pr.approximator(seed, base)
    dpl, dql = linear_bounds(pr, seed, base, near, dl_l)
    cost, bound = costs_and_bounds(t, t.obstacle_tables(), params, pr.linear_frames(tb_l, dl_l, base, near), dpl, dql)
    pl, _ = h.fitness(abi.FK_LINEAR, seed, params, near, base)
    want, bnd = tc.sums(t, cost, bound)[0]
    err = np.abs(pl - want)
    r = stats.ratio("linear primary", err, np.maximum(bnd, 1e-300), name)
    assert r <= 1.0, "%s: linearised primary fitness off by %.3g, bound %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))])
    h.close()
    return pa, pl


def symmetry(make_solver, stats, n=200):
    """goal (L, O) and goal (O, L) state the same distances: under exact FK they agree within the sum of their bounds (the summation order differs: not bit for bit)"""
    model = with_points(pr2_like(), (RW, *balls(5, 31, 0.05, 0.2)), (LW, *balls(4, 32, 0.05, 0.2)))
    res = []
    for goal in (SelfClearanceGoal(RW, LW, 0.01), SelfClearanceGoal(LW, RW, 0.01)):
        t, h, pr, seed, genes = setup(make_solver, model, "all", [goal], "symmetry", n)
        pa, cost, bound, _, _ = exact_against(t, h, pr, seed, t.pack_params(), genes, stats, "symmetry")
        res.append((pa, bound[:, 0] + C * U * pa))
        h.close()
    (a, ba), (b, bb) = res
    assert np.any(a > 0.0) and np.all(np.abs(a - b) <= ba + bb), np.abs(a - b).max()


def streamed(make_solver, device_arrays):
    """bioik_stream_fitness_device (genes [unit][D][pop]) gives the bits of bioik_eval_fitness, exact FK, on the same library"""
    model, group, goals = function_cases()["two_goals_one_tip"]
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
        assert np.array_equal(got[u], want) and np.any(want > 0.0), u
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
class NoLink(bl.RawBase):
    """goal 0 names no link"""

    def __init__(self, model, group, goals, raw):
        super().__init__(model, group, goals, raw)
        self._goal_descs[0].link = -1


def refusals(make_solver, lib):
    """every row of the table of include/bioik_hip.h (BIOIK_GOAL_SELF_CLEARANCE) with its status code and a word of its message, which names the goal's index"""
    assert lib.bioik_goal_param_count(20) == 1 and lib.bioik_goal_param_count(19) == 1 and lib.bioik_goal_param_count(18) == -1 and lib.bioik_goal_param_count(21) == -1
    ok = pair_model(3, 4)
    goal = lambda **kw: SelfClearanceGoal(RW, LW, 0.0, **kw)  # noqa: E731
    sec = goal()
    sec.secondary_ = True

    def spoiled(link, how):
        m = pair_model(3, 4)
        if how == "disks":
            m.add_collision_cylinder(link, 0.03, 0.1)
        elif how == "cylinder":  # a marker row, r == -1: what a shape that is no set of spheres leaves behind (tests/touch_cases.py: cylinder_model, unresolved_mesh_model)
            m.add_collision_unsupported(link, "cylinder")
        else:
            m.link_meshes.setdefault(m.link_index(link), []).append(("package://x/pad.stl", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)))
            m.meshes_resolved.discard(m.link_index(link))  # (a <mesh> that is only named: the spheres beside it were not its vertices)
        return m
    tree, links = bl.held_limit_model()
    for l in links:
        tree.add_collision_points(l, [[0.0, 0.0, 0.0]], [0.05])
    held = lambda pairs: [SelfClearanceGoal(links[2 * i], links[2 * i + 1], 0.0) for i in range(pairs)]  # noqa: E731
    n_links = ok.n_links
    rows = [
        (ProblemTemplate(ok, "all", [SelfClearanceGoal(RW, "", 0.0)]), abi.ERR_INVALID_ARGUMENT, ("goal 0", "other link")),  # goal_base_link NULL
        (bl.ExplicitWorld(ok, "all", [SelfClearanceGoal(RW, "", 0.0)]), abi.ERR_INVALID_ARGUMENT, ("goal 0", "other link")),  # -1
        (ProblemTemplate(ok, "all", [PositionGoal(LW, base_link=RW), SelfClearanceGoal(RW, "", 0.0)]), abi.ERR_INVALID_ARGUMENT, ("goal 1", "other link")),
        (NoLink(ok, "all", [goal()], [ok.link_index(LW)]), abi.ERR_INVALID_ARGUMENT, ("goal 0", "names no link")),
        (ProblemTemplate(ok, "all", [SelfClearanceGoal(RW, RW, 0.0)]), abi.ERR_INVALID_ARGUMENT, ("goal 0", "own link")),
        (ProblemTemplate(with_points(pr2_like(), (LW, *balls(4, 1, 0.1, 0.2))), "all", [goal()]), abi.ERR_INVALID_ARGUMENT, ("goal 0", "the goal's link has no collision points")),
        (ProblemTemplate(with_points(pr2_like(), (RW, *cc.spheres(3, 1))), "all", [goal()]), abi.ERR_INVALID_ARGUMENT, ("goal 0", "the other link has no collision points")),
        (ProblemTemplate(spoiled(RW, "disks"), "all", [goal()]), abi.ERR_UNSUPPORTED, ("goal 0", "the goal's link carries disks")),
        (ProblemTemplate(spoiled(LW, "disks"), "all", [goal()]), abi.ERR_UNSUPPORTED, ("goal 0", "the other link carries disks")),
        (ProblemTemplate(spoiled(RW, "cylinder"), "all", [goal()]), abi.ERR_UNSUPPORTED, ("goal 0", "radius -1")),
        (ProblemTemplate(spoiled(LW, "mesh"), "all", [goal()]), abi.ERR_UNSUPPORTED, ("goal 0", "the other link in", "radius -1")),
        (ProblemTemplate(pair_model(abi.MAX_TOUCH_POINTS + 1, 4), "all", [goal()]), abi.ERR_UNSUPPORTED, ("goal 0", "BIOIK_MAX_TOUCH_POINTS")),
        (ProblemTemplate(pair_model(3, abi.MAX_OBSTACLES + 1), "all", [goal()]), abi.ERR_UNSUPPORTED, ("goal 0", "BIOIK_MAX_OBSTACLES")),
        (ProblemTemplate(ok, "all", [PositionGoal(RW), sec]), abi.ERR_UNSUPPORTED, ("goal 1", "secondary")),
        (ProblemTemplate(tree, "g", held(abi.MAX_HELD_FRAMES + 1)), abi.ERR_UNSUPPORTED, ("goal %d" % abi.MAX_HELD_FRAMES, "BIOIK_MAX_HELD_FRAMES")),
        (bl.RawBase(ok, "all", [goal()], [n_links]), abi.ERR_NOT_FOUND, ("goal 0", "base link")),
    ]
    for t, code, words in rows:
        try:
            make_solver(t)
        except solver.BioIKError as e:
            assert e.code == code and all(w in str(e) and w in lib.bioik_last_error().decode() for w in words), (code, words, e.code, str(e))
        else:
            raise AssertionError("accepted: %s %s" % (code, words))
    make_solver(ProblemTemplate(tree, "g", held(abi.MAX_HELD_FRAMES))).close()  # (the limit itself is accepted)
    # a struct_size that ends in front of goal_base_link: the caller cannot have named an other link
    t = ProblemTemplate(ok, "all", [goal()])
    md, model = ok.desc(), ctypes.c_void_p()
    assert lib.bioik_model_create(ctypes.byref(md), 0, ctypes.byref(model)) == abi.OK
    d, prob = t.desc(), ctypes.c_void_p()
    d.struct_size = abi.ProblemDesc.goal_base_link.offset
    assert lib.bioik_problem_create(model, ctypes.byref(d), ctypes.byref(prob)) == abi.ERR_INVALID_ARGUMENT and b"goal 0" in lib.bioik_last_error() and b"struct_size" in lib.bioik_last_error()
    lib.bioik_model_destroy(model)
    # the obstacle-table calls know no table of such a goal
    h = make_solver(t)
    for call in (lambda: h.set_obstacles(0, cc.scene(2, 2)), lambda: h.obstacle_count(0)):
        try:
            call()
        except solver.BioIKError as e:
            assert e.code == abi.ERR_INVALID_ARGUMENT and "not a CLEARANCE goal" in str(e) and "not a CLEARANCE goal" in lib.bioik_last_error().decode(), str(e)
        else:
            raise AssertionError("accepted: an obstacle table on a SelfClearanceGoal")
    # BIOIK_MODE_JAC: refused by the solve call, nothing launched, the outputs keep their pattern; the gradient modes run
    n = 3
    seeds = np.tile(np.asarray(ok.default_positions(), dtype=np.float64), (n, 1))
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
SOLVE = dict(cc.SOLVE)  # population 128, 64 steps, 4 islands, seed 5 (dtwist: the default, 1e-5)
DTWIST = 1e-5
MARGIN = 0.01
VARIANTS = ("primary", "gd", "ranked", "bounded")
CROSS = 0.2  # (m) how far the right wrist's target lies to the LEFT of the left wrist's
FOREARM_SPHERES = ([[0.05, 0, 0], [0.15, 0, 0], [0.25, 0, 0]], [0.08, 0.08, 0.08])


def solve_model():
    return with_points(pr2_like(), (RF, *FOREARM_SPHERES), (LF, *FOREARM_SPHERES))


def solve_template(goals=True):
    return ProblemTemplate(solve_model(), "all", [PositionGoal(RW), PositionGoal(LW)] + ([SelfClearanceGoal(RF, LF, MARGIN)] if goals else []))


def forearm_depth(m, x, margin=0.0):
    """how deep the forearms' spheres are inside one another at the full variable vectors x (n, V): long double on the float64 frames of bio_ik_amd.robot"""
    from bio_ik_amd.robot import link_transform
    out = np.zeros(len(x))
    for i, xi in enumerate(x):
        a, b = (np.asarray(link_transform(m, m.link_index(l), xi)) for l in (LF, RF))
        p, q = bl.relative(a[None, :3], a[None, 3:], b[None, :3], b[None, 3:])
        pen, _, _ = cc.pair_penetrations(margin, p, q, m.collision_points(m.link_index(RF)), m.collision_points(m.link_index(LF)))
        out[i] = float(pen.max())
    return out


@functools.lru_cache(maxsize=None)
def targets_and_seeds(n, seed):
    """per query the two wrist positions of a random configuration whose arms CROSS (the right wrist left of the left one, both in front of the chest) and whose
    forearms are clear of one another by twice the margin, so an answer exists; the solve starts from another random configuration.  Computed once, read-only."""
    from bio_ik_amd.robot import link_transform
    m = solve_model()
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    torso = m.variable_index("torso_lift_joint")
    targets, seeds = [], []
    while len(targets) < n:
        x = lo + (hi - lo) * rng.random(m.n_variables)
        x[torso] = 0.1
        r, l = (np.asarray(link_transform(m, m.link_index(k), x))[:3] for k in (RW, LW))
        if not (r[0] > 0.35 and l[0] > 0.35 and r[1] - l[1] > CROSS and abs(r[2] - l[2]) < 0.25):
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


def queries(t, n=N_QUERIES, seed=13):
    targets, seeds = targets_and_seeds(n, seed)
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        params[:, off:off + len(g.params())] = g.params()[None]
    params[:, 0:3], params[:, 3:6] = targets[:, :3], targets[:, 3:]
    return seeds.copy(), params


def solve_bounds(t, seeds):
    """the bounded variant: the model's own bounds, the continuous forearm and wrist rolls narrowed to +-2.5 around 0 (every seed moved inside)"""
    m = t.model
    lo, hi = np.array(m.var_min, dtype=np.float64), np.array(m.var_max, dtype=np.float64)
    for name in ("r_forearm_roll_joint", "r_wrist_roll_joint", "l_forearm_roll_joint", "l_wrist_roll_joint"):
        v = m.variable_index(name)
        lo[v], hi[v] = -2.5, 2.5
    seeds = np.clip(seeds, lo[None], hi[None])
    return np.ascontiguousarray(seeds), (np.tile(lo, (len(seeds), 1)), np.tile(hi, (len(seeds), 1)))


def run(h, t, variant, seeds, params):
    p = abi.default_solve_params(mode="gd", max_steps=64, islands=4, random_seed=5) if variant == "gd" else abi.default_solve_params(**SOLVE)
    if variant == "ranked":
        return p, h.solve_batch_ranked(p, seeds, params, 2, 0.0)
    if variant == "bounded":
        seeds, bounds = solve_bounds(t, seeds)
        return p, h.solve_batch(p, seeds, params, bounds=bounds)
    return p, h.solve_batch(p, seeds, params)


def verify_solve(t, h, seeds, params, sol, fit, suc):
    """on the returned joint values, recomputed in long double: every row flagged a success has no pair of spheres deeper than dtwist / weight (the success rule:
    weighted cost < dtwist^2, and the cost is at least the deepest pair's square) up to the bound of the cost, and its PositionGoals within 3 dtwist^2; the fitness is
    the long-double cost within its bound.  Returns per row the deepest penetration over the SelfClearanceGoals at their margins (0 without one)."""
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    inactive = np.setdiff1d(np.arange(h.V), pr.active)
    deepest = np.zeros(sol.shape[0])
    for i in range(sol.shape[0]):
        b = rr.Bounds(pr, sol[i:i + 1].astype(np.float64))
        depth = {}
        cost, bound = costs_and_bounds(t, {}, params[i], tc.exact_frames(pr, sol[i], sol[i:i + 1, pr.active]), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, depth)
        assert np.array_equal(sol[i, inactive], seeds[i, inactive])
        if suc[i]:
            for k, g in enumerate(t.goals):
                limit = (3 if g.opcode == abi.GOAL_POSITION else 1) * DTWIST ** 2
                assert float(cost[0, k]) < limit + bound[0, k], (i, k, float(cost[0, k]), bound[0, k])
                if k in depth:
                    assert (depth[k][0] * g.getWeight()) ** 2 < DTWIST ** 2 + bound[0, k], (i, k, depth[k][0])
        want = float(cost[0].sum())
        assert abs(fit[i] - want) <= bound[0].sum() + C * U * want, (i, fit[i], want)
        deepest[i] = max([depth[k][0] for k in depth] + [0.0])
    return deepest


STEERING = {}
# found on the host simulator (= the device, bit for bit) and asserted as found, not hoped for: WITHOUT the SelfClearanceGoal this many of the 16 answers have forearms more
# than 1 cm inside one another; WITH it this many of the 16 succeed
WITHOUT_PENETRATING, WITH_SUCCESS = 10, 16


def whole_solve(make_solver, variant="primary"):
    """Returns (solver, template, seeds, params, solve parameters, results) for bit comparisons."""
    t = solve_template()
    h = make_solver(t)
    seeds, params = queries(t)
    p, res = run(h, t, variant, seeds, params)
    if variant == "bounded":
        seeds, (lo, hi) = solve_bounds(t, seeds)
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
    """non-vacuity, on the answers `with_goals` of the primary variant: the same queries WITHOUT the SelfClearanceGoal return WITHOUT_PENETRATING (>= 4) answers whose
    forearms are more than 1 cm inside one another; WITH it all 16 succeed, and a success has no pair deeper than dtwist / weight (verify_solve)"""
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


def mapping_independence(make_solver, monkeypatch, steps=SOLVE["max_steps"], n=N_QUERIES, islands=SOLVE["islands"], population=SOLVE["population"]):
    """the whole-solve case gives the same bits under every lane mapping the BIOIK_SOLVE_* switches can force for it (the general kernel flavour: the switches that
    name a lean mapping are passed over by the launcher)"""
    t = solve_template()
    h = make_solver(t)
    seeds, params = queries(t, n)
    for fk in (abi.FK_EXACT, abi.FK_LINEAR):
        p = abi.default_solve_params(population=population, max_steps=steps, islands=islands, random_seed=5, fk_mode=fk)
        base = h.solve_batch(p, seeds, params)
        for env in tc.MAPPINGS:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = h.solve_batch(p, seeds, params)
            for k in env:
                monkeypatch.delenv(k)
            assert all(np.array_equal(a, b) for a, b in zip(base, got)), (fk, env)
    h.close()
