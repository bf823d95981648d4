"""ClearanceGoal (opcode 19) on the library under test: the GPU suite (tests/test_gpu_clearance.py) and the host simulator (tests/test_hostsim_clearance.py) run
these cases.  `make_solver(template)` makes a bio_ik_amd.solver.HipSolver of the library under test.

The pin is the formula of the goal restated in long double from its definition (include/bioik_hip.h: BIOIK_GOAL_CLEARANCE), on the long-double forward kinematics
of tests/np_fk.py -- not the oracle (it does not know the opcode) and not the kernel.  With the link's frame (p, q), its points (v_i, r_i) and the obstacle rows
(c_j, R_j):

    w_i = p + rotate(q, v_i)     s_ij = (margin + r_i) + R_j     pen = s_ij > 0 ? max(0, s_ij - |w_i - c_j|) : 0     cost = weight^2 sum_i sum_j pen^2

Error bound, built like the one of tests/touch_cases.py (same C and U, the same FK bounds dp / dq of a tip and the same `rot` of a rotated vector).  max(0, .) is
1-Lipschitz, so per pair

    |pen - pen_exact| <= e_ij = dp + (rot + C U) |v_i| + C U (|s_ij| + |c_j| + |w_i|)         pen^2: sq_bound(pen, e_ij)

summed over the pairs and multiplied by weight^2.  The running sum of the n m squares, all >= 0, rounds once per pair that adds something, each time by at most U of
a partial sum that is at most the cost: (C + n m) U cost on top (C U alone is the arithmetic of one square; a table of 256 obstacles against 17 points is 4352
additions into one sum, not "a few").

A secondary link goal reads the null frame (p = 0, q = 0: ik_base.h:163, as every secondary link goal of this library does), known exactly: there w_i = v_i."""
import functools
import types

import numpy as np

import np_goals
import random_robot_cases as rr
import touch_cases as tc
from bio_ik_amd import ClearanceGoal, PoseGoal, PositionGoal, ProblemTemplate, TouchGoal, abi, pr2_like, solver
from bio_ik_amd.robot import link_transform
from np_fk import LD

C, U = rr.C, rr.U
CAP = abi.MAX_OBSTACLES
TIP, TIP_L, FOREARM = "r_wrist_roll_link", "l_wrist_roll_link", "r_forearm_link"
POINT_COUNTS, OBSTACLE_COUNTS = (1, 2, 3, 17), (0, 1, 2, 3, 9, CAP)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------
def world_points(p, q, pts):
    """w (n, points, 3) in long double for frames p (n, 3), q (n, 4): p + rotate(q, v), q as it is"""
    pts = np.asarray(pts, dtype=LD).reshape(-1, 4)
    return np.stack([np.asarray(p, dtype=LD) + tc.rotate_ld(q, pts[i, :3]) for i in range(pts.shape[0])], axis=1)


def pair_penetrations(margin, p, q, pts, obs):
    """pen (n, points, obstacles), s (points, obstacles) and w (n, points, 3) of the formula above: long double"""
    pts = np.asarray(pts, dtype=LD).reshape(-1, 4)
    obs = np.asarray(obs, dtype=LD).reshape(-1, 4)
    w = world_points(p, q, pts)
    s = (LD(margin) + pts[:, 3])[:, None] + obs[None, :, 3]
    d = np.sqrt(((w[:, :, None, :] - obs[None, None, :, :3]) ** 2).sum(axis=3))
    pen = np.where(s[None] > 0, np.maximum(LD(0), s[None] - d), LD(0))
    return pen, s, w


def clearance(margin, p, q, pts, obs, d_p, d_q):
    """the unweighted cost (n,) in long double and its bound (n,) for frames known to d_p / d_q (n,); also the deepest penetration (n,)"""
    n = np.asarray(p).shape[0]
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 4)
    pts64 = np.asarray(pts, dtype=np.float64).reshape(-1, 4)
    if obs.shape[0] == 0:
        return np.zeros(n, dtype=LD), np.zeros(n), np.zeros(n)
    pen, s, w = pair_penetrations(margin, p, q, pts, obs)
    qn = np.linalg.norm(np.asarray(q, dtype=np.float64), axis=1)
    rot = 2 * d_q * (1 + qn * qn)
    vn = np.linalg.norm(pts64[:, :3], axis=1)
    wn = np.linalg.norm(np.asarray(w, dtype=np.float64), axis=2)
    e = (d_p[:, None, None] + (rot[:, None, None] + C * U) * vn[None, :, None] +
         C * U * (np.abs(np.asarray(s, dtype=np.float64))[None] + np.linalg.norm(obs[:, :3], axis=1)[None, None, :] + wn[:, :, None]))
    pen64 = np.asarray(pen, dtype=np.float64)
    cost = (pen * pen).sum(axis=(1, 2))
    bound = rr.sq_bound(pen64, e).sum(axis=(1, 2)) + (C + pen.shape[1] * pen.shape[2]) * U * np.asarray(cost, dtype=np.float64)
    return cost, bound, pen64.max(axis=(1, 2))


# ---- models and scenes --------------------------------------------------------------------------------------------------------------------------------------
def spheres(n, seed, scale=0.08, rmax=0.05):
    rng = np.random.default_rng(seed)
    return rng.uniform(-scale, scale, size=(n, 3)), rng.uniform(0.0, rmax, size=n)


def arm_with(n_points, seed=1, link=TIP):
    m = pr2_like()
    m.add_collision_points(link, *spheres(n_points, seed))
    return m


def scene(m, seed, rmin=0.02, rmax=0.15, box=((0.2, -0.7, 0.4), (0.9, 0.3, 1.3))):
    """m obstacle rows in the right arm's workspace: some individuals of a random population penetrate some of them"""
    rng = np.random.default_rng(1000 + seed)
    return np.hstack([rng.uniform(box[0], box[1], size=(m, 3)), rng.uniform(rmin, rmax, size=(m, 1))])


def function_cases():
    """name -> (model, group, goals): the trip counts of both loops, the cap, the branch in all its states, the tables' places in the buffer, the goal tables"""
    out = {}
    for n in POINT_COUNTS:
        for m in OBSTACLE_COUNTS:
            out["points_%d_obstacles_%d" % (n, m)] = (arm_with(n, n), "right_arm", [ClearanceGoal(TIP, 0.01, scene(m, 7 * n + m, rmin=0.15, rmax=0.35))])
    far = scene(9, 1) + np.array([100.0, 0, 0, 0])
    out["all_far"] = (arm_with(3), "right_arm", [ClearanceGoal(TIP, 0.02, far)])
    out["all_penetrating"] = (arm_with(3), "right_arm", [ClearanceGoal(TIP, 0.02, scene(9, 2, rmin=5.0, rmax=6.0))])
    out["some_individuals"] = (arm_with(3), "right_arm", [ClearanceGoal(TIP, 0.0, [[0.6, -0.2, 0.8, 0.35]])])  # (one ball in the middle of the workspace: the branch diverges)
    out["negative_margin"] = (arm_with(3), "right_arm", [ClearanceGoal(TIP, -20.0, scene(9, 2, rmin=5.0, rmax=6.0))])  # s <= 0 for every pair
    # d2 = 0 exactly: a secondary goal reads the null frame, where w_i = v_i; two of the obstacles sit on two of the points
    m = arm_with(3)
    v = m.collision_points(m.link_index(TIP))
    sec = ClearanceGoal(TIP, 0.01, [[v[0][0], v[0][1], v[0][2], 0.03], [1.0, 1.0, 1.0, 0.1], [v[2][0], v[2][1], v[2][2], 0.0]], weight=0.8)
    sec.secondary_ = True
    out["centred_secondary"] = (m, "right_arm", [PositionGoal(TIP, (0.6, -0.2, 0.8)), sec])
    # two goals on two links of the branching model with different tables, the first one's points and block behind a TouchGoal's points in the buffer
    m = pr2_like()
    m.add_collision_points(TIP, *spheres(5, 21))
    m.add_collision_points(TIP_L, *spheres(2, 22))
    m.add_collision_points(FOREARM, *spheres(4, 23))  # (a link no goal names, in front of both in link order)
    out["two_links_behind_touch"] = (m, "all", [TouchGoal(TIP, (0.55, -0.2, 0.7), (0.2, -0.3, 0.9), weight=0.7), ClearanceGoal(TIP, 0.03, scene(9, 3), weight=1.3),
                                                ClearanceGoal(TIP_L, 0.0, scene(2, 4, box=((0.2, -0.3, 0.4), (0.9, 0.7, 1.3))), weight=0.6)])
    out["beside_pose_goal"] = (arm_with(3), "right_arm", [PoseGoal(TIP, (0.6, -0.2, 0.8), (0.1, 0.2, 0.3, 0.9)), ClearanceGoal(TIP, 0.01, scene(9, 5))])
    out["weight"] = (arm_with(3), "right_arm", [ClearanceGoal(TIP, 0.01, scene(9, 6), weight=0.37)])
    return out


# ---- costs and bounds ---------------------------------------------------------------------------------------------------------------------------------------
def costs_and_bounds(t, tables, params, frames, dp, dq, depth=None):
    """weighted cost (n, n_goals) in long double and its bound, for frames {link: (p, q)} known to dp / dq {link: (n,)}.  `tables`: {goal index: obstacle rows}, what
    the handle holds.  The goals that are no ClearanceGoal: tests/touch_cases.py.  `depth` (optional dict): per clearance goal its deepest penetration (n,)"""
    n = next(iter(frames.values()))[0].shape[0]
    cost = np.zeros((n, len(t.goals)), dtype=LD)
    bound = np.zeros((n, len(t.goals)))
    others = [k for k, g in enumerate(t.goals) if g.opcode != abi.GOAL_CLEARANCE]
    if others:
        shim = types.SimpleNamespace(goals=[t.goals[k] for k in others], param_offsets=[t.param_offsets[k] for k in others], model=t.model)
        c, b = tc.costs_and_bounds(shim, None, params, frames, dp, dq)
        cost[:, others], bound[:, others] = c, b
    for k, (g, off) in enumerate(zip(t.goals, t.param_offsets)):
        if g.opcode != abi.GOAL_CLEARANCE:
            continue
        link = t.model.link_index(g.link_name())
        if g.isSecondary():
            p, q, d_p, d_q = np.zeros((n, 3), dtype=LD), np.zeros((n, 4), dtype=LD), np.zeros(n), np.zeros(n)
        else:
            (p, q), d_p, d_q = frames[link], dp[link], dq[link]
        c, b, deep = clearance(params[off], p, q, t.model.collision_points(link), tables[k], np.broadcast_to(d_p, (n,)), np.broadcast_to(d_q, (n,)))
        w2 = LD(g.getWeight()) ** 2
        cost[:, k] = c * w2
        bound[:, k] = float(w2) * b + C * U * np.abs(np.asarray(cost[:, k], dtype=np.float64))
        if depth is not None:
            depth[k] = deep
    return cost, bound


def population(model, pr, rng, n):
    lo, hi = np.asarray(model.var_min), np.asarray(model.var_max)
    seed = lo + (hi - lo) * rng.random(model.n_variables)
    X = lo + (hi - lo) * rng.random((n, model.n_variables))
    return seed, np.ascontiguousarray(X[:, pr.active])


def exact_fitness_against(t, h, pr, tables, seed, params, genes, stats, name):
    """bioik_eval_fitness, exact FK, against the restatement with the tables `tables`; returns the device's primary fitness and the restatement's costs"""
    b = rr.Bounds(pr, pr.full(seed, genes).astype(np.float64))
    cost, bound = costs_and_bounds(t, tables, params, tc.exact_frames(pr, seed, genes), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m})
    pa, sa = h.fitness(abi.FK_EXACT, seed, params, genes)
    for got, (want, bnd), what in zip((pa, sa), tc.sums(t, cost, bound), ("exact primary", "exact secondary")):
        err = np.abs(got - want)
        r = stats.ratio(what, err, np.maximum(bnd, 1e-300), name)
        worst = int(np.argmax(err / np.maximum(bnd, 1e-300)))
        assert r <= 1.0, "%s: %s fitness off by %.3g, bound %.3g (row %d)" % (name, what, err.max(), bnd[worst], worst)
    return pa, sa, cost, b


def function_level(make_solver, name, stats, n=200):
    """bioik_eval_fitness in both FK modes and bioik_eval_check against the restatement; the worst error / bound ratios go to `stats`"""
    model, group, goals = function_cases()[name]
    t = ProblemTemplate(model, group, goals)
    h = make_solver(t)
    tables = t.obstacle_tables()
    for k, rows in tables.items():
        assert h.obstacle_count(k) == len(rows), (name, k)
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    rng = np.random.default_rng(sum(map(ord, name)))
    seed, genes = population(model, pr, rng, n)
    params = t.pack_params()
    pa, sa, cost, b = exact_fitness_against(t, h, pr, tables, seed, params, genes, stats, name)
    clear = [k for k, g in enumerate(t.goals) if g.opcode == abi.GOAL_CLEARANCE]
    if name in ("all_far", "negative_margin") or name.endswith("_obstacles_0"):
        assert np.all(pa == 0.0) and np.all(np.asarray(cost[:, clear], dtype=np.float64) == 0.0), name  # exactly nothing, not "small"
    if name.startswith("points_") and not name.endswith("_obstacles_0"):
        assert np.any(pa > 0.0), name  # (every case of the grid takes the branch somewhere)
    if name == "all_penetrating":
        pen, _, _ = pair_penetrations(params[0], *tc.exact_frames(pr, seed, genes)[model.link_index(TIP)], model.collision_points(model.link_index(TIP)), tables[0])
        assert np.all(np.asarray(pen, dtype=np.float64) > 1.0), name
    if name == "some_individuals":
        hit = int(np.count_nonzero(pa > 0.0))
        assert n // 20 < hit < n - n // 20, (name, hit)  # lanes that take the branch beside lanes that do not
    if name == "centred_secondary":
        assert np.all(sa > 0.0) and np.ptp(sa) == 0.0, name  # (the null frame: the same number for every individual)
    # the success test (problem.cpp:327-334, the default branch): weighted cost < min(dpos, dtwist)^2 for every primary goal.  Per row the margin of every
    # primary ClearanceGoal is set from the row's own least gap, min_ij |w_i - c_j| - r_i - R_j: 1 mm below it nothing penetrates and the cost is 0, provably a
    # success; 1 cm above it some pair penetrates by 1 cm and the weighted cost is at least weight^2 1e-4 > 1e-6, provably none
    prim = [k for k, g in enumerate(t.goals) if not g.isSecondary()]
    if all(t.goals[k].opcode == abi.GOAL_CLEARANCE and len(tables[k]) for k in prim):
        sp = abi.default_solve_params(dpos=-1.0, drot=-1.0, dtwist=1e-3)
        fr = tc.exact_frames(pr, seed, genes)
        rows = list(range(0, n, max(n // 16, 1)))
        hits = 0
        for j, i in enumerate(rows):
            P1 = params.copy()
            f1 = {l: (fr[l][0][i:i + 1], fr[l][1][i:i + 1]) for l in fr}
            for k in prim:
                link = model.link_index(t.goals[k].link_name())
                pts = np.asarray(model.collision_points(link), dtype=LD).reshape(-1, 4)
                obs = np.asarray(tables[k], dtype=LD)
                w = world_points(f1[link][0], f1[link][1], pts)[0]
                gap = np.sqrt(((w[:, None, :] - obs[None, :, :3]) ** 2).sum(axis=2)) - pts[:, 3:4] - obs[None, :, 3]
                P1[t.param_offsets[k]] = float(gap.min()) + (-1e-3 if j % 2 == 0 else 1e-2 / abs(t.goals[k].getWeight()))
            c1, b1 = costs_and_bounds(t, tables, P1, f1, {l: b.dp(l)[i:i + 1] for l in b.m}, {l: b.dq(l)[i:i + 1] for l in b.m})
            ok = int(h.check(sp, seed, P1, genes[i:i + 1])[0])
            sure_yes = all(float(c1[0, k]) + b1[0, k] < 1e-6 for k in prim)
            sure_no = any(float(c1[0, k]) - b1[0, k] >= 1e-6 for k in prim)
            assert sure_yes == (j % 2 == 0) and sure_no == (j % 2 == 1), (name, i, [float(c1[0, k]) for k in prim])
            assert ok == (1 if sure_yes else 0), (name, i, ok, [float(c1[0, k]) for k in prim])
            hits += ok
        assert hits == (len(rows) + 1) // 2, (name, hits)
    # linearised phenotypes around a base: tip + sum of delta (gene - base), the quaternion not renormalised; frames and their bounds as
    # tests/touch_cases.py builds them
    base = genes[0]
    near = np.ascontiguousarray(base + 0.02 * rng.normal(size=(max(n // 8, 4), len(pr.active))))
    tb_l, dl_l = pr.approximator(seed, base)
    lf = pr.linear_frames(tb_l, dl_l, base, near)
    bi = rr.Bounds(pr, pr.full(seed, base[None]).astype(np.float64))
    bl = rr.Bounds(pr, pr.full(seed, near).astype(np.float64))
    dv = np.abs(near - base[None])
    dp, dq = {}, {}
    for ti, tl in enumerate(pr.tips):
        tabs = np.full(len(pr.active), 2 * bl.dq(tl)[0] * (bl.lam[tl][0] + 1) * 4)
        mag = np.abs(np.asarray(dl_l[ti], dtype=np.float64)).max(axis=1)
        dp[tl] = bi.dp(tl)[0] + dv @ tabs + C * U * (dv @ mag)
        dq[tl] = bi.dq(tl)[0] + dv @ tabs + C * U * (dv @ mag)
    cost, bound = costs_and_bounds(t, tables, params, lf, dp, dq)
    pl, _ = h.fitness(abi.FK_LINEAR, seed, params, near, base)
    want, bnd = tc.sums(t, cost, bound)[0]
    err = np.abs(pl - want)
    r = stats.ratio("linear primary", err, np.maximum(bnd, 1e-300), name)
    assert r <= 1.0, "%s: linearised primary fitness off by %.3g, bound %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))])
    h.close()


def streamed(make_solver, device_arrays):
    """bioik_stream_fitness_device (genes [unit][D][pop]) gives the bits of bioik_eval_fitness, exact FK, on the same library"""
    model, group, goals = function_cases()["two_links_behind_touch"]
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


def table_updates(make_solver, stats, lib, n=200):
    """one handle: 200 rows, then 3, then 0, then 256; after each the fitness against the restatement with THAT table; a refused call leaves the table in place"""
    model = arm_with(3)
    t = ProblemTemplate(model, "right_arm", [ClearanceGoal(TIP, 0.01)])
    h = make_solver(t)
    assert h.obstacle_count(0) == 0
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    seed, genes = population(model, pr, np.random.default_rng(17), n)
    params = t.pack_params()
    before = None
    for step, m in enumerate((200, 3, 0, CAP)):
        rows = scene(m, 40 + step)
        h.set_obstacles(0, rows)
        assert h.obstacle_count(0) == m
        pa, _, _, _ = exact_fitness_against(t, h, pr, {0: rows}, seed, params, genes, stats, "update_%d" % m)
        assert (m == 0) == bool(np.all(pa == 0.0)), m
        assert before is None or not np.array_equal(before, pa), m
        before = pa
        for bad, code, word in ((np.vstack([scene(2, 1), [[0, 0, np.nan, 0.1]]]), abi.ERR_INVALID_ARGUMENT, "not finite"),
                                (np.vstack([scene(2, 1), [[0, 0, np.inf, 0.1]]]), abi.ERR_INVALID_ARGUMENT, "not finite"),
                                (np.vstack([scene(2, 1), [[0, 0, 0, -0.1]]]), abi.ERR_INVALID_ARGUMENT, "radius"),
                                (scene(CAP + 1, 1), abi.ERR_UNSUPPORTED, "BIOIK_MAX_OBSTACLES")):
            try:
                h.set_obstacles(0, bad)
            except solver.BioIKError as e:
                assert e.code == code and word in str(e) and word in lib.bioik_last_error().decode(), (code, str(e))
            else:
                raise AssertionError("accepted: " + word)
            assert h.obstacle_count(0) == m
            assert np.array_equal(h.fitness(abi.FK_EXACT, seed, params, genes)[0], pa), (m, word)
    h.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def refusals(make_solver, lib):
    assert lib.bioik_goal_param_count(19) == 1 and lib.bioik_goal_param_count(18) == -1
    disks = pr2_like()
    disks.add_collision_points(TIP, *spheres(2, 1))
    disks.add_collision_cylinder(TIP, 0.03, 0.1)
    many = pr2_like()
    many.add_collision_points(TIP, *spheres(abi.MAX_TOUCH_POINTS + 1, 1))
    based = ClearanceGoal(TIP, 0.0)
    based.setBaseLinkName(FOREARM)
    for model, goal, code, word in ((pr2_like(), ClearanceGoal(TIP), abi.ERR_INVALID_ARGUMENT, "no collision points"),
                                    (arm_with(3, link=FOREARM), ClearanceGoal(TIP), abi.ERR_INVALID_ARGUMENT, "no collision points"),
                                    (disks, ClearanceGoal(TIP), abi.ERR_UNSUPPORTED, "disks"),
                                    (tc.cylinder_model(), ClearanceGoal(TIP), abi.ERR_UNSUPPORTED, "radius -1"),
                                    (tc.unresolved_mesh_model(), ClearanceGoal(TIP), abi.ERR_UNSUPPORTED, "radius -1"),
                                    (many, ClearanceGoal(TIP), abi.ERR_UNSUPPORTED, "BIOIK_MAX_TOUCH_POINTS"),
                                    (arm_with(3), based, abi.ERR_UNSUPPORTED, "base link")):
        try:
            make_solver(ProblemTemplate(model, "right_arm", [goal]))
        except solver.BioIKError as e:
            assert e.code == code and word in str(e) and word in lib.bioik_last_error().decode(), (code, word, str(e))
        else:
            raise AssertionError("accepted: " + word)
    # the calls: an index out of range, a goal that is no CLEARANCE goal
    h = make_solver(ProblemTemplate(arm_with(3), "right_arm", [PositionGoal(TIP), ClearanceGoal(TIP, 0.0, scene(3, 1))]))
    assert h.obstacle_count(1) == 3
    for k, word in ((0, "not a CLEARANCE goal"), (2, "out of range"), (-1, "out of range")):
        for call in (lambda: h.set_obstacles(k, scene(2, 2)), lambda: h.obstacle_count(k)):
            try:
                call()
            except solver.BioIKError as e:
                assert e.code == abi.ERR_INVALID_ARGUMENT and word in str(e) and word in lib.bioik_last_error().decode(), (k, str(e))
            else:
                raise AssertionError("accepted: goal index %d" % k)
    assert h.obstacle_count(1) == 3
    h.close()


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------------------------
N_QUERIES = 16
SOLVE = dict(population=128, max_steps=64, islands=4, random_seed=5)  # (dtwist: the default, 1e-5)
DTWIST = 1e-5
MARGIN = 0.01
# one scene: a column of spheres in front of the targets, between the shoulder and where the hand is asked to go
COLUMN = np.array([[0.45, -0.25, z, 0.07] for z in np.arange(0.45, 1.26, 0.1)])
VARIANTS = ("primary", "secondary", "gd", "ranked", "bounded")


def solve_model():
    m = pr2_like()
    m.add_collision_points(FOREARM, [[0.05, 0, 0], [0.15, 0, 0], [0.25, 0, 0]], [0.05, 0.05, 0.05])
    m.add_collision_points(TIP, [[0.0, 0, 0], [0.08, 0, 0]], [0.045, 0.04])
    return m


def solve_template(variant="primary", clearance=True):
    goals = [PositionGoal(TIP)]
    if clearance:
        goals += [ClearanceGoal(FOREARM, MARGIN, COLUMN), ClearanceGoal(TIP, MARGIN, COLUMN)]
    if variant == "secondary":
        sec = ClearanceGoal(TIP, MARGIN, [[0.05, 0.0, 0.0, 0.03]], weight=0.5)  # (the null frame, w_i = v_i: a constant > 0, as every secondary link goal is one)
        sec.secondary_ = True
        goals.append(sec)
    return ProblemTemplate(solve_model(), "right_arm", goals)


@functools.lru_cache(maxsize=None)
def targets_and_seeds(n, seed):
    """per query a target: the tip position of a random configuration that is itself clear of the column by twice the margin (so an answer exists), behind the
    column as seen from the shoulder; the solve starts from another random configuration.  Computed once and shared (read-only)."""
    m = solve_model()
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    torso = m.variable_index("torso_lift_joint")
    targets, seeds = [], []
    while len(targets) < n:
        x = lo + (hi - lo) * rng.random(m.n_variables)
        x[torso] = 0.1  # (no variable of the group)
        tip = np.asarray(link_transform(m, m.link_index(TIP), x))
        if not (tip[0] > 0.55 and -0.5 < tip[1] < 0.0):
            continue
        free = all(g.evaluate(link_transform(m, m.link_index(g.link_name()), x), m.collision_points(m.link_index(g.link_name()))) == 0.0
                   for g in (ClearanceGoal(FOREARM, 2 * MARGIN, COLUMN), ClearanceGoal(TIP, 2 * MARGIN, COLUMN)))
        if not free:
            continue
        s = lo + (hi - lo) * rng.random(m.n_variables)
        s[torso] = 0.1
        targets.append(tip[:3])
        seeds.append(s)
    targets, seeds = np.ascontiguousarray(targets), np.ascontiguousarray(seeds)
    targets.setflags(write=False), seeds.setflags(write=False)
    return targets, seeds


def queries(t, n=N_QUERIES, seed=11):
    targets, seeds = targets_and_seeds(n, seed)
    seeds = seeds.copy()
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        params[:, off:off + len(g.params())] = g.params()[None]
        if g.opcode == abi.GOAL_POSITION:
            params[:, off:off + 3] = targets
    return seeds, params


def solve_bounds(t, seeds):
    """the bounded variant: the model's own bounds, the two continuous joints narrowed to +-2.5 around 0 (every seed moved inside)"""
    m = t.model
    lo, hi = np.array(m.var_min, dtype=np.float64), np.array(m.var_max, dtype=np.float64)
    for name in ("r_forearm_roll_joint", "r_wrist_roll_joint"):
        v = m.variable_index(name)
        lo[v], hi[v] = -2.5, 2.5
    seeds = np.clip(seeds, lo[None], hi[None])
    return np.ascontiguousarray(seeds), (np.tile(lo, (len(seeds), 1)), np.tile(hi, (len(seeds), 1)))


def verify_solve(t, h, tables, seeds, params, sol, fit, suc):
    """condition 1 on the returned joint values, recomputed in long double: every row flagged a success has every primary goal's weighted cost below what the
    success test allows plus its bound -- a ClearanceGoal dtwist^2 (the default branch), the PositionGoal 3 dtwist^2 (its test: every component of the twist below
    dtwist).  Returns per row the deepest penetration over the clearance goals (0 without one)."""
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    n = sol.shape[0]
    deepest = np.zeros(n)
    for i in range(n):
        g1 = sol[i:i + 1, pr.active]
        b = rr.Bounds(pr, sol[i:i + 1].astype(np.float64))
        depth = {}
        cost, bound = costs_and_bounds(t, tables, params[i], tc.exact_frames(pr, sol[i], g1), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, depth)
        prim = [k for k, g in enumerate(t.goals) if not g.isSecondary()]
        sec = [k for k, g in enumerate(t.goals) if g.isSecondary()]
        assert np.array_equal(sol[i, np.setdiff1d(np.arange(h.V), pr.active)], seeds[i, np.setdiff1d(np.arange(h.V), pr.active)])
        if suc[i]:
            for k in prim:
                limit = (3 if t.goals[k].opcode == abi.GOAL_POSITION else 1) * DTWIST ** 2
                assert float(cost[0, k]) < limit + bound[0, k], (i, k, float(cost[0, k]), bound[0, k])
        want = float(cost[0, prim].sum()) + (float(cost[0, sec].sum()) if suc[i] else 0.0)
        bnd = bound[0, prim].sum() + (bound[0, sec].sum() if suc[i] else 0.0) + C * U * want
        assert abs(fit[i] - want) <= bnd, (i, fit[i], want, bnd)
        deepest[i] = max([depth[k][0] for k in prim if k in depth] + [0.0])
    return deepest


def penetration(sol, margin=0.0):
    """per row of full variable vectors how deep the link spheres are inside the column (margin 0: real contact)"""
    m = solve_model()
    out = np.zeros(len(sol))
    for i, x in enumerate(sol):
        for link in (FOREARM, TIP):
            f = np.asarray(link_transform(m, m.link_index(link), x))
            pen, _, _ = pair_penetrations(margin, f[None, :3], f[None, 3:], m.collision_points(m.link_index(link)), COLUMN)
            out[i] = max(out[i], float(pen.max()))
    return out


def run(h, t, variant, seeds, params):
    if variant == "gd":
        p = abi.default_solve_params(mode="gd", max_steps=64, islands=4, random_seed=5)
    else:
        p = abi.default_solve_params(**SOLVE)
    if variant == "ranked":
        return p, h.solve_batch_ranked(p, seeds, params, 2, 0.0)
    if variant == "bounded":
        seeds, bounds = solve_bounds(t, seeds)
        return p, h.solve_batch(p, seeds, params, bounds=bounds)
    return p, h.solve_batch(p, seeds, params)


def whole_solve(make_solver, variant="primary"):
    """Returns (solver, template, seeds, params, solve parameters, results) for bit comparisons."""
    t = solve_template(variant)
    h = make_solver(t)
    tables = t.obstacle_tables()
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
            verify_solve(t, h, tables, seeds[rows], params[rows], sol[rows, r], fit[rows, r], suc[rows, r])
    else:
        verify_solve(t, h, tables, seeds, params, res[0], res[1], res[2])
    if variant == "primary":
        steering(make_solver, seeds, p, res)
    return h, t, seeds, params, p, res


def steering(make_solver, seeds, p, with_goals):
    """condition 2, on the answers `with_goals` of the primary variant: the same queries WITHOUT the ClearanceGoals return at least four answers that are more than
    1 cm inside the column; WITH them at least one of those four queries succeeds -- and a success is clear of the column by the margin (condition 1), so at margin 0
    it touches nothing.  The counts go to STEERING (the test prints them)."""
    t0 = solve_template(clearance=False)
    h0 = make_solver(t0)
    _, params0 = queries(t0)
    sol0, _, suc0, _ = h0.solve_batch(p, seeds, params0)
    h0.close()
    sol1, _, suc1, _ = with_goals
    deep0, deep1 = penetration(sol0), penetration(sol1)
    bad = np.nonzero(deep0 > 0.01)[0]
    STEERING.update(without_penetrating=int(len(bad)), without_success=int(suc0.sum()), with_success=int(suc1.sum()), with_penetrating=int(np.count_nonzero(deep1 > 0.01)))
    assert len(bad) >= 4, (len(bad), deep0)
    four = bad[np.argsort(-deep0[bad])][:4]
    STEERING.update(with_success_of_four=int(suc1[four].sum()))
    assert suc1[four].sum() >= 1, (four, suc1)
    assert np.all(deep1[suc1 != 0] == 0.0)


STEERING = {}


def mapping_independence(make_solver, monkeypatch, variants=("primary", "secondary"), steps=SOLVE["max_steps"], n=N_QUERIES, islands=SOLVE["islands"]):
    """the whole-solve case gives the same bits under every lane mapping the BIOIK_SOLVE_* switches can force for it (a problem with a ClearanceGoal runs in the
    general kernel flavour: the switches that name a lean mapping are passed over by the launcher)"""
    for variant in variants:
        t = solve_template(variant)
        h = make_solver(t)
        seeds, params = queries(t, n)
        for fk in (abi.FK_EXACT, abi.FK_LINEAR):
            p = abi.default_solve_params(population=128, max_steps=steps, islands=islands, random_seed=5, fk_mode=fk)
            base = h.solve_batch(p, seeds, params)
            for env in tc.MAPPINGS:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                got = h.solve_batch(p, seeds, params)
                for k in env:
                    monkeypatch.delenv(k)
                assert all(np.array_equal(a, b) for a, b in zip(base, got)), (variant, fk, env)
        h.close()
