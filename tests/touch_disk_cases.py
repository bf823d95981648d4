"""TouchGoal (opcode 17) on links that carry DISKS -- the ends of cylinders, the bases of cones -- beside or instead of points: the GPU suite
(tests/test_gpu_touch_disks.py) and the host simulator (tests/test_hostsim_touch_disks.py) run these cases; tests/touch_cases.py has the points-only ones and
the helpers taken from it here.  `make_solver(template)` makes a bio_ik_amd.solver.HipSolver of the library under test.

The pin is the formula of the goal restated in long double from its definition (include/bioik_hip.h: BIOIK_GOAL_TOUCH) on the long-double forward kinematics
of tests/np_fk.py:

    n_l = rotate(conjugate(q), normal)
    d = min( min_i (n_l . v_i - r_i),  min_j (n_l . c_j - r_j |n_l x a_j|) ) - normal . (position - p)          cost = weight^2 d^2

and tests/test_touch_disks_api.py checks the disk term of that restatement against something that is not the formula: the brute-force minimum over points
sampled on the rim.

Error bound.  That of tests/touch_cases.py (same C and U, dp / dq of the tip, rot = 2 dq (1 + |q|^2) of a vector of length one turned by the frame's
quaternion) with two changes.  (1) A disk's term is  n_l . c_j - r_j |n_l x a_j|.  The computed n_l is off by at most rot |n|, |n| = 1: that moves n_l . c_j
by at most rot |c_j| and, since |(n_l + e) x a| differs from |n_l x a| by at most |e x a| <= |e| for the unit axis, r_j |n_l x a_j| by at most rot r_j; the
roundings of the three FMAs of n_l . c_j are C U |c_j| as for a point.  So where the points' bound has max |v_i| the disks have |c_j| + r_j, and the maximum
over both kinds stands in its place.  (2) The cross product (three products, three fused multiply-adds), its squared norm, the correctly rounded root and
the product with r_j are a dozen roundings, each relative to a quantity of size at most |n_l| |a_j| ~ 1 (the norm's error is absolute in the components, not
relative to the norm: right where n_l is parallel to a_j the norm is small and its relative error is not): C U r_j, the maximum over j.  Together

    |d - d_exact| <= dp |n| + (rot + C U) max(max_i |v_i|, max_j (|c_j| + r_j)) + C U (|position| + |p|) + C U max_j r_j
    cost: sq_bound(|d|, that) weight^2 + C U cost

The minimum itself adds nothing: min is exact, and |min f - min g| <= max |f - g|."""
import ctypes as Ct

import numpy as np

import np_goals
import random_robot_cases as rr
import touch_cases as tc
from bio_ik_amd import PoseGoal, PositionGoal, ProblemTemplate, TouchGoal, abi, pr2_like, solver
from np_fk import LD

C, U, CAP, TIP, TIP_L, BOX = tc.C, tc.U, tc.CAP, tc.TIP, tc.TIP_L, tc.BOX
IDENT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------
def disk_support(n_l, disks):
    """n_l (n, 3) long double, disks [m][8] -> (n, m): n_l . c_j - r_j |n_l x a_j|"""
    dk = np.asarray(disks, dtype=LD).reshape(-1, 8)
    n_l = np.asarray(n_l, dtype=LD)
    rim = np.sqrt((np.cross(n_l[:, None, :], dk[None, :, 4:7]) ** 2).sum(axis=2))
    return n_l @ dk[:, :3].T - dk[None, :, 3] * rim


def touch_parts(P, p, q, points, disks):
    """the terms of the minimum, points first then disks (n, n_points + n_disks), and the plane's offset normal . (position - p) (n,): long double"""
    P = np.asarray(P, dtype=LD)
    pts = np.asarray(points, dtype=LD).reshape(-1, 4)
    conj = np.asarray(q, dtype=LD) * np.array([-1, -1, -1, 1], dtype=LD)
    n_l = tc.rotate_ld(conj, P[3:6])
    parts = np.hstack([n_l @ pts[:, :3].T - pts[None, :, 3], disk_support(n_l, disks)])
    return parts, (P[None, :3] - np.asarray(p, dtype=LD)) @ P[3:6]


def touch_distance(P, p, q, points, disks):
    """d of the formula above for frames p (n, 3), q (n, 4): long double"""
    parts, off = touch_parts(P, p, q, points, disks)
    return parts.min(axis=1) - off


# ---- models -------------------------------------------------------------------------------------------------------------------------------------------------
def random_disks(n, seed, scale=0.08, rmax=0.05):
    rng = np.random.default_rng(1000 + seed)
    a = rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    return np.hstack([rng.uniform(-scale, scale, size=(n, 3)), rng.uniform(0.0, rmax, size=(n, 1)), a])


def arm_with_disks(disks=None, points=None, radii=None, link=TIP, points_first=True):
    m = pr2_like()
    if points is not None and points_first:
        m.add_collision_points(link, points, radii)
    if disks is not None:
        m.add_collision_disks(link, disks)
    if points is not None and not points_first:
        m.add_collision_points(link, points, radii)
    return m


O_CYL = (0.03, -0.02, 0.01) + tuple(tc.quat_from_rpy(0.4, -0.7, 0.2))
O_CONE = (0.01, 0.02, -0.01) + tuple(tc.quat_from_rpy(-0.3, 0.5, 1.1))
O_CONE_DOWN = (0.0, -0.01, 0.02) + tuple(tc.quat_from_rpy(3.0, 0.2, -0.4))  # (nearly upside down)
CYL = (0.03, 0.12)  # radius, length


def arm_with_cylinder():
    m = pr2_like()
    m.add_collision_cylinder(TIP, CYL[0], CYL[1], O_CYL)
    return m


def function_cases():
    """name -> (model, group, goals): the shapes where the disk loop, the zero-trip point loop, the table offsets and the goal tables can go wrong"""
    out = {}
    P0, N0 = (0.55, -0.2, 0.7), (0.2, -0.3, 0.9)
    for n in (1, 2, 3, 5):  # no points: zero trips of the point loop, and the odd disk
        out["disks_%d" % n] = (arm_with_disks(random_disks(n, n)), "right_arm", [TouchGoal(TIP, P0, N0)])
    m = pr2_like()  # the disks' table offset lies behind 8 points
    m.add_collision_box(TIP, BOX)
    m.add_collision_cylinder(TIP, CYL[0], CYL[1], O_CYL)
    out["cylinder_beside_box"] = (m, "right_arm", [TouchGoal(TIP, P0, N0)])
    for name, o in (("cone", O_CONE), ("cone_down", O_CONE_DOWN)):  # (function_level asserts that the apex is lowest in some rows and the base in others)
        m = pr2_like()
        m.add_collision_cone(TIP, 0.04, 0.10, o)
        out[name] = (m, "right_arm", [TouchGoal(TIP, P0, N0)])
    # a disk of radius 0 at the place of a point: both terms are n_l . v, the disk's by another sequence of operations
    spot = (0.09, -0.05, 0.07)
    out["zero_radius_disk_at_point"] = (arm_with_disks([spot + (0.0, 0.6, 0.0, 0.8)], np.vstack([[spot], tc.random_points(2, 9, 0.01)])), "right_arm", [TouchGoal(TIP, P0, N0)])
    # the minimum at the first / the last disk for EVERY direction: a disk that swallows everything (a sphere of 0.3 fits between its rim and the rest)
    small, big = random_disks(4, 7, 0.01, 0.01), [(0.0, 0.0, 0.0, 0.5, 0.0, 0.6, 0.8)]
    pts = tc.random_points(3, 8, 0.01)
    out["swallow_first"] = (arm_with_disks(np.vstack([big, small]), pts), "right_arm", [TouchGoal(TIP, P0, N0)])
    out["swallow_last"] = (arm_with_disks(np.vstack([small, big]), pts), "right_arm", [TouchGoal(TIP, P0, N0)])
    # the normal parallel to the axis IN THE LINK FRAME: a secondary goal reads the null frame, so n_l = normal = (0, 0, 1) exactly and |n_l x a| = 0 exactly
    m = pr2_like()
    m.add_collision_cylinder(TIP, CYL[0], CYL[1])
    sec = TouchGoal(TIP, (0.1, 0.2, 0.3), (0, 0, 1), weight=0.8)
    sec.secondary_ = True
    out["parallel_secondary"] = (m, "right_arm", [PositionGoal(TIP, (0.6, -0.2, 0.8)), sec])
    m = pr2_like()  # two goals on two links of the branching model, each with disks: the second goal's rows start behind the first's points AND disks
    m.add_collision_cylinder(TIP_L, 0.02, 0.15, O_CONE)
    m.add_collision_points(TIP_L, tc.random_points(3, 21))
    m.add_collision_box(TIP, BOX)
    m.add_collision_cylinder(TIP, CYL[0], CYL[1], O_CYL)
    m.add_collision_cylinder("r_forearm_link", 0.05, 0.3)  # (a link no goal names, in front of both in link order)
    out["two_links"] = (m, "all", [TouchGoal(TIP, P0, N0, weight=0.7), TouchGoal(TIP_L, (0.5, 0.3, 0.6), (0, 0, 1), weight=1.3)])
    out["at_the_cap"] = (arm_with_disks(random_disks(3, 3), tc.random_points(CAP - 3, 4)), "right_arm", [TouchGoal(TIP, P0, N0)])
    return out


# ---- costs and bounds ---------------------------------------------------------------------------------------------------------------------------------------
def costs_and_bounds(t, pr, params, frames, dp, dq, dist=None):
    """touch_cases.costs_and_bounds with the disks of the link in the TouchGoal's distance and in its bound (the module's docstring)"""
    n = next(iter(frames.values()))[0].shape[0]
    cost = np.zeros((n, len(t.goals)), dtype=LD)
    bound = np.zeros((n, len(t.goals)))
    for k, (g, off) in enumerate(zip(t.goals, t.param_offsets)):
        P = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[g.opcode]], dtype=np.float64)
        link = t.model.link_index(g.link_name())
        if g.isSecondary():
            p, q, d_p, d_q = np.zeros((n, 3), dtype=LD), np.zeros((n, 4), dtype=LD), np.zeros(n), np.zeros(n)
        else:
            (p, q), d_p, d_q = frames[link], dp[link], dq[link]
        w2 = LD(g.getWeight()) ** 2
        p64, q64 = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
        if g.opcode == abi.GOAL_TOUCH:
            pts, dks = t.model.collision_points(link), t.model.collision_disks(link)
            d = touch_distance(P, p, q, pts, dks)
            c = d * d
            qn = np.linalg.norm(q64, axis=1)
            rot = 2 * d_q * (1 + qn * qn)
            reach = max([0.0] + list(np.linalg.norm(pts[:, :3], axis=1)) + list(np.linalg.norm(dks[:, :3], axis=1) + dks[:, 3]))
            dr = d_p * np.linalg.norm(P[3:6]) + (rot + C * U) * reach + C * U * (np.linalg.norm(P[:3]) + np.linalg.norm(p64, axis=1)) + C * U * max([0.0] + list(dks[:, 3]))
            b = rr.sq_bound(np.abs(np.asarray(d, dtype=np.float64)), dr)
            if dist is not None:
                dist[k] = (abs(g.getWeight()) * np.abs(np.asarray(d, dtype=np.float64)), abs(g.getWeight()) * dr)
        else:
            c = np_goals.link_cost(g.opcode, np.asarray(P, dtype=LD), p, q)
            b = rr.sq_bound(np.linalg.norm(p64 - P[:3], axis=1), d_p)
            if g.opcode == abi.GOAL_POSE:
                b = b + P[7] ** 2 * rr.sq_bound(np.minimum(np.linalg.norm(P[3:7] - q64, axis=1), np.linalg.norm(P[3:7] + q64, axis=1)), d_q)
        cost[:, k] = c * w2
        bound[:, k] = float(w2) * b + C * U * np.abs(np.asarray(cost[:, k], dtype=np.float64))
    return cost, bound


def function_level(make_solver, name, stats, n=200):
    """bioik_eval_fitness in both FK modes and bioik_eval_check against the restatement, as touch_cases.function_level; the worst error / bound ratios go to
    `stats`"""
    model, group, goals = function_cases()[name]
    t = ProblemTemplate(model, group, goals)
    h = make_solver(t)
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    rng = np.random.default_rng(sum(map(ord, name)))
    lo, hi = np.asarray(model.var_min), np.asarray(model.var_max)
    seed = lo + (hi - lo) * rng.random(model.n_variables)
    X = lo + (hi - lo) * rng.random((n, model.n_variables))
    genes = np.ascontiguousarray(X[:, pr.active])
    params = t.pack_params()
    b = rr.Bounds(pr, pr.full(seed, genes).astype(np.float64))
    fr = tc.exact_frames(pr, seed, genes)
    cost, bound = costs_and_bounds(t, pr, params, fr, {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m})
    if name.startswith("cone"):  # the apex (the link's one point, column 0) is the lowest part in some rows and the base disk (column 1) in others
        link = model.link_index(TIP)
        parts, _ = touch_parts(params[:6], fr[link][0], fr[link][1], model.collision_points(link), model.collision_disks(link))
        apex_lowest = int((parts[:, 0] < parts[:, 1]).sum())
        assert parts.shape[1] == 2 and 0 < apex_lowest < n, (name, apex_lowest)
    if name == "parallel_secondary":  # |n_l x a| is zero exactly: the restatement's value is the lower end's n . c, with no radius in it
        d = touch_distance(params[3:9], np.zeros((1, 3)), np.zeros((1, 4)), model.collision_points(TIP), model.collision_disks(TIP))
        assert d[0] == LD(-0.5 * CYL[1]) - LD(params[5])
    pa, sa = h.fitness(abi.FK_EXACT, seed, params, genes)
    for got, (want, bnd), what in zip((pa, sa), tc.sums(t, cost, bound), ("exact primary", "exact secondary")):
        err = np.abs(got - want)
        print("%s: %s worst error %.3g, bound there %.3g" % (name, what, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))]))
        r = stats.ratio(what, err, np.maximum(bnd, 1e-300), name)
        assert r <= 1.0, "%s: %s fitness off by %.3g, bound %.3g (row %d)" % (name, what, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))], int(np.argmax(err / np.maximum(bnd, 1e-300))))
    # the success test (problem.cpp:327-334, the default branch): weighted cost < min(dpos, dtwist)^2 for every primary goal; half of the rows get a plane
    # through their own lowest point (a cost of nothing), and a decision may differ from the restatement's only inside the bound
    if all(g.opcode == abi.GOAL_TOUCH for g in goals if not g.isSecondary()):
        sp = abi.default_solve_params(dpos=-1.0, drot=-1.0, dtwist=1e-3)
        hits = 0
        rows = list(range(0, n, max(n // 16, 1)))
        for j, i in enumerate(rows):
            P1 = params.copy()
            for g, off in zip(t.goals, t.param_offsets):
                if not g.isSecondary() and j % 2 == 0:
                    link = model.link_index(g.link_name())
                    d = touch_distance(np.concatenate([np.zeros(3), P1[off + 3:off + 6]]), fr[link][0][i:i + 1], fr[link][1][i:i + 1], model.collision_points(link),
                                       model.collision_disks(link))
                    P1[off:off + 3] = np.asarray(d[0] * np.asarray(P1[off + 3:off + 6], dtype=LD), dtype=np.float64)  # d(position) = d(0) - normal . position = 0
            f1 = {l: (fr[l][0][i:i + 1], fr[l][1][i:i + 1]) for l in fr}
            c1, b1 = costs_and_bounds(t, pr, P1, f1, {l: b.dp(l)[i:i + 1] for l in b.m}, {l: b.dq(l)[i:i + 1] for l in b.m})
            ok = int(h.check(sp, seed, P1, genes[i:i + 1])[0])
            prim = [k for k, g in enumerate(t.goals) if not g.isSecondary()]
            sure_yes = all(float(c1[0, k]) + b1[0, k] < 1e-6 for k in prim)
            sure_no = any(float(c1[0, k]) - b1[0, k] >= 1e-6 for k in prim)
            assert not (sure_yes and ok != 1) and not (sure_no and ok != 0), (name, i, ok, [float(c1[0, k]) for k in prim])
            hits += ok
        assert 0 < hits < len(rows), (name, hits)
    # linearised phenotypes around a base, frames and their bounds as touch_cases.function_level builds them
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
    cost, bound = costs_and_bounds(t, pr, params, lf, dp, dq)
    pl, _ = h.fitness(abi.FK_LINEAR, seed, params, near, base)
    want, bnd = tc.sums(t, cost, bound)[0]
    err = np.abs(pl - want)
    print("%s: linear primary worst error %.3g, bound there %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))]))
    r = stats.ratio("linear primary", err, np.maximum(bnd, 1e-300), name)
    assert r <= 1.0, "%s: linearised primary fitness off by %.3g, bound %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))])
    h.close()


def streamed(make_solver, device_arrays):
    """bioik_stream_fitness_device (genes [unit][D][pop]) gives the bits of bioik_eval_fitness, exact FK, on the cylinder beside the box"""
    model, group, goals = function_cases()["cylinder_beside_box"]
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


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def model_create(lib, desc):
    handle = Ct.c_void_p()
    rc = lib.bioik_model_create(Ct.byref(desc), 0, Ct.byref(handle))
    if rc == abi.OK:
        lib.bioik_model_destroy(handle)
    return rc, lib.bioik_last_error().decode()


def refusals(make_solver, lib):
    touch = [TouchGoal(TIP, (0, 0, 0), (0, 0, 1))]
    # malformed disks: bioik_model_create refuses them (the Python setters would too, so the rows are put into the descriptor behind their back)
    m = arm_with_cylinder()
    n_links, link = m.n_links, m.link_index(TIP)
    first = np.zeros(n_links + 1, dtype=np.int32)
    first[link + 1:] = 1
    for row in ((0, 0, 0, -0.5, 0, 0, 1, 0), (0, 0, 0, -1.0, 0, 0, 1, 0), (0, 0, 0, 0.1, 0, 0, 1.001, 0), (0, 0, 0, 0.1, 0, 0, 0, 0), (0, np.nan, 0, 0.1, 0, 0, 1, 0),
                (0, 0, 0, np.inf, 0, 0, 1, 0), (0, 0, 0, 0.1, np.nan, 0, 1, 0)):
        d = m.desc()
        bad = np.array([row], dtype=np.float64)
        d.link_disk_first, d.link_disks = abi.iptr(first), abi.dptr(bad)
        rc, text = model_create(lib, d)
        assert rc == abi.ERR_INVALID_ARGUMENT and "disk" in text, (row, rc, text)
    d = m.desc()
    d.link_disks = None  # one of the pair without the other
    assert model_create(lib, d)[0] == abi.ERR_INVALID_ARGUMENT
    # one row over the cap, in points + disks together (the model at the cap is a function-level case)
    for model, code, word in ((arm_with_disks(random_disks(3, 3), tc.random_points(CAP - 2, 4)), abi.ERR_UNSUPPORTED, "BIOIK_MAX_TOUCH_POINTS"),
                              (arm_with_disks(random_disks(CAP + 1, 3)), abi.ERR_UNSUPPORTED, "BIOIK_MAX_TOUCH_POINTS"),
                              (arm_with_disks(random_disks(2, 1), link="r_forearm_link"), abi.ERR_INVALID_ARGUMENT, "no collision points"),
                              (marker_beside_disk_model(), abi.ERR_UNSUPPORTED, "marker")):
        try:
            make_solver(ProblemTemplate(model, "right_arm", touch))
        except solver.BioIKError as e:
            assert e.code == code and word in str(e) and word in lib.bioik_last_error().decode(), (code, str(e))
        else:
            raise AssertionError("accepted: " + word)
    # a PoseGoal on a model with disks (and on one with a marker beside a disk): accepted
    make_solver(ProblemTemplate(arm_with_cylinder(), "right_arm", [PoseGoal(TIP)])).close()
    make_solver(ProblemTemplate(marker_beside_disk_model(), "right_arm", [PoseGoal(TIP)])).close()
    # the three struct_size forms.  Full: the disks are there.  Without the disks' pair: the box's points are there, a cylinder link has nothing.  Without
    # either pair: no shapes at all.  A size between two of them: refused.
    both = pr2_like()
    both.add_collision_box(TIP, BOX)
    both.add_collision_cylinder(TIP_L, CYL[0], CYL[1])
    for size, ok_box, ok_cyl in ((Ct.sizeof(abi.ModelDesc), True, True), (abi.ModelDesc.link_disk_first.offset, True, False), (abi.ModelDesc.link_point_first.offset, False, False)):
        d = both.desc()
        d.struct_size = size
        handle = Ct.c_void_p()
        assert lib.bioik_model_create(Ct.byref(d), 0, Ct.byref(handle)) == abi.OK, lib.bioik_last_error().decode()
        for tip, group, ok in ((TIP, "right_arm", ok_box), (TIP_L, "left_arm", ok_cyl)):
            pd, prob = ProblemTemplate(both, group, [TouchGoal(tip, (0, 0, 0), (0, 0, 1))]).desc(), Ct.c_void_p()
            rc = lib.bioik_problem_create(handle, Ct.byref(pd), Ct.byref(prob))
            assert rc == (abi.OK if ok else abi.ERR_INVALID_ARGUMENT), (size, tip, rc)
            if rc == abi.OK:
                lib.bioik_problem_destroy(prob)
            else:
                assert "no collision points" in lib.bioik_last_error().decode()
        lib.bioik_model_destroy(handle)
    for size in (abi.ModelDesc.link_point_first.offset + 4, abi.ModelDesc.link_point_first.offset + 8, abi.ModelDesc.link_disk_first.offset + 4,
                 abi.ModelDesc.link_disk_first.offset + 8, Ct.sizeof(abi.ModelDesc) + 8):
        d = both.desc()
        d.struct_size = size
        assert model_create(lib, d)[0] == abi.ERR_INVALID_ARGUMENT, size


def marker_beside_disk_model():
    """a cylinder that was converted and a shape that was not, on one link: scoring the cylinder alone would be a silent approximation"""
    m = arm_with_cylinder()
    m.add_collision_unsupported(TIP, "cone")
    return m


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------------------------
N_QUERIES, SOLVE = tc.N_QUERIES, tc.SOLVE


def lowest_point(pts, dks, R, p, n):
    """the lowest point along the unit normal n of the hull of points (spheres) and disks moved by the frame (R, p): long double"""
    n = np.asarray(n, dtype=LD)
    n_l = R.T @ n
    cand, val = [], []
    for v in np.asarray(pts, dtype=LD).reshape(-1, 4):
        cand.append(p + R @ v[:3] - v[3] * n)
        val.append(n_l @ v[:3] - v[3])
    for k in np.asarray(dks, dtype=LD).reshape(-1, 8):
        flat = n_l - (n_l @ k[4:7]) * k[4:7]  # the normal's part in the disk's plane: the rim's lowest point lies against it
        ln = np.sqrt(flat @ flat)
        rim = k[:3] - (k[3] / ln) * flat if ln > 0 else k[:3]
        cand.append(p + R @ rim)
        val.append(n_l @ rim)
    return cand[int(np.argmin(val))]


def reachable_queries(t, h, n=N_QUERIES, seed=11):
    """touch_cases.reachable_queries for any shape: per query a random configuration inside the limits, its tip frame in long double, a random unit normal, and
    `position` at the lowest point of the link's shapes along the normal -- the plane then touches the shape at that configuration; the solve starts from
    another random configuration"""
    m = t.model
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    target = lo + (hi - lo) * rng.random((n, m.n_variables))
    seeds = np.ascontiguousarray(lo + (hi - lo) * rng.random((n, m.n_variables)))
    seeds[:, :] = np.where(np.isin(np.arange(m.n_variables), pr.active)[None], seeds, target)  # (inactive variables: the target's, the torso among them)
    normals = rng.normal(size=(n, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    link = m.link_index(TIP)
    R, p = pr.frames(target[0], target[:, pr.active])
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        for i in range(n):
            if g.opcode == abi.GOAL_TOUCH:
                low = lowest_point(m.collision_points(link), m.collision_disks(link), R[link][i], p[link][i], normals[i])
                params[i, off:off + 3], params[i, off + 3:off + 6] = np.asarray(low, dtype=np.float64), normals[i]
            else:  # the PositionGoal beside a secondary touch goal: the link's origin at the target
                params[i, off:off + 3] = np.asarray(p[link][i], dtype=np.float64)
    return seeds, params


def verify_solve(t, h, seeds, params, sol, fit, suc, min_success):
    """touch_cases.verify_solve on this module's costs_and_bounds: the asserts of a whole solve on the returned joint values, recomputed in long double"""
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    n = sol.shape[0]
    won = 0
    for i in range(n):
        g1 = sol[i:i + 1, pr.active]
        b = rr.Bounds(pr, sol[i:i + 1].astype(np.float64))
        dist = {}
        cost, bound = costs_and_bounds(t, pr, params[i], tc.exact_frames(pr, sol[i], g1), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, dist)
        prim = [k for k, g in enumerate(t.goals) if not g.isSecondary()]
        sec = [k for k, g in enumerate(t.goals) if g.isSecondary()]
        assert np.array_equal(sol[i, np.setdiff1d(np.arange(h.V), pr.active)], seeds[i, np.setdiff1d(np.arange(h.V), pr.active)])
        touch = [k for k in prim if k in dist]
        if suc[i]:  # weighted |d| below dtwist = 1e-5 within the bound of its recomputation
            for k in touch:
                assert dist[k][0][0] < 1e-5 + dist[k][1][0], (i, k, dist[k])
        elif len(touch) == len(prim):
            assert any(dist[k][0][0] >= 1e-5 - dist[k][1][0] for k in touch), (i, dist)
        want = float(cost[0, prim].sum()) + (float(cost[0, sec].sum()) if suc[i] else 0.0)
        bnd = bound[0, prim].sum() + (bound[0, sec].sum() if suc[i] else 0.0) + C * U * want
        assert abs(fit[i] - want) <= bnd, (i, fit[i], want, bnd)
        won += int(suc[i])
    print("%d of %d queries solved" % (won, n))
    assert won >= min_success, "%d of %d queries solved" % (won, n)
    return won


def solve_template(variant):
    m = arm_with_cylinder()
    if variant == "secondary":
        sec = TouchGoal(TIP, (0, 0, 0), (0, 0, 1))
        sec.secondary_ = True
        return ProblemTemplate(m, "right_arm", [PositionGoal(TIP), sec])
    return ProblemTemplate(m, "right_arm", [TouchGoal(TIP, (0, 0, 0), (0, 0, 1))])


def whole_solve(make_solver, variant="primary"):
    """variant: primary | secondary (beside a PositionGoal) | gd | ranked (bioik_solve_batch_ranked, k = 2).  Returns (solver, ..., results) for bit comparisons."""
    t = solve_template(variant)
    h = make_solver(t)
    seeds, params = reachable_queries(t, h)
    if variant == "gd":
        p = abi.default_solve_params(mode="gd", max_steps=SOLVE["max_steps"], islands=SOLVE["islands"], random_seed=SOLVE["random_seed"])
    else:
        p = abi.default_solve_params(**SOLVE)
    if variant == "ranked":
        sol, fit, suc, steps, count = h.solve_batch_ranked(p, seeds, params, 2, 0.0)
        assert count.min() >= 1
        best = h.solve_batch(p, seeds, params)
        assert all(np.array_equal(a[:, 0], b) for a, b in zip((sol, fit, suc, steps), best))  # row 0: the plain answer, bit for bit
        for r in range(2):
            rows = count > r
            verify_solve(t, h, seeds[rows], params[rows], sol[rows, r], fit[rows, r], suc[rows, r], N_QUERIES // 2 if r == 0 else 0)
        res = (sol, fit, suc, steps, count)
    else:
        res = h.solve_batch(p, seeds, params)
        verify_solve(t, h, seeds, params, res[0], res[1], res[2], N_QUERIES // 2)
    return h, t, seeds, params, p, res


def mapping_independence(make_solver, monkeypatch, variants=("primary", "secondary"), steps=8, n=8, islands=2):
    """a shortened whole-solve case (8 queries, 8 steps, two islands by default) gives the same bits under every lane mapping of touch_cases.MAPPINGS"""
    for variant in variants:
        t = solve_template(variant)
        h = make_solver(t)
        seeds, params = reachable_queries(t, h, n)
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
