"""TouchGoal (opcode 17) on the library under test: the GPU suite (tests/test_gpu_touch.py) and the host simulator (tests/test_hostsim_touch.py) run these
cases.  `make_solver(template)` makes a bio_ik_amd.solver.HipSolver of the library under test.

The pin is the formula of the goal restated in long double from its definition (include/bioik_hip.h: BIOIK_GOAL_TOUCH), on the long-double forward kinematics
of tests/np_fk.py -- not the oracle (it does not know the opcode: the reference's TouchGoal needs FCL and is compiled out of oracle/_ref) and not the kernel:

    n_l = rotate(conjugate(q), normal)     d = min_i (n_l . v_i - r_i) - normal . (position - p)     cost = weight^2 d^2

Error bound, built like those of tests/random_robot_cases.py (same C and U, the same FK bounds dp / dq of a tip and the same `rot` of a rotated vector):

    |d - d_exact| <= dp |n| + (rot + C U) max|v_i| + C U (|position| + |p|)        cost: sq_bound(|d|, that) weight^2 + C U cost

A secondary link goal reads the null frame (p = 0, q = 0: ik_base.h:163, as every secondary link goal of this library does), known exactly."""
import numpy as np

import np_goals
import random_robot_cases as rr
from bio_ik_amd import PoseGoal, PositionGoal, ProblemTemplate, TouchGoal, abi, pr2_like, solver
from bio_ik_amd.robot import quat_from_rpy
from np_fk import LD, quat_from_rot_batch

C, U = rr.C, rr.U
CAP = abi.MAX_TOUCH_POINTS
TIP, TIP_L = "r_wrist_roll_link", "l_wrist_roll_link"
BOX = (0.10, 0.06, 0.04)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------------
def rotate_ld(q, v):
    """v turned by the quaternion q (n, 4) as it is, unit or not: v + 2 (w u x v + u x (u x v)), u = q.xyz"""
    q = np.asarray(q, dtype=LD)
    v = np.broadcast_to(np.asarray(v, dtype=LD), (q.shape[0], 3))
    u, w = q[:, :3], q[:, 3:4]
    t = np.cross(u, v)
    return v + 2 * (w * t + np.cross(u, t))


def touch_distance(P, p, q, points):
    """d of the formula above for frames p (n, 3), q (n, 4): long double"""
    P = np.asarray(P, dtype=LD)
    pts = np.asarray(points, dtype=LD).reshape(-1, 4)
    conj = np.asarray(q, dtype=LD) * np.array([-1, -1, -1, 1], dtype=LD)
    n_l = rotate_ld(conj, P[3:6])
    support = np.min(n_l @ pts[:, :3].T - pts[None, :, 3], axis=1)
    return support - (P[None, :3] - np.asarray(p, dtype=LD)) @ P[3:6]


def expected_box(size, origin=None):
    """the 8 corners of a URDF box moved by its origin (xyz, rpy) into the link frame, by the rotation matrix of its rpy in long double"""
    h = np.asarray(size, dtype=LD) / 2
    c = np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=LD)
    return np.hstack([move(c, origin), np.zeros((8, 1), dtype=LD)])


def move(pts, origin):
    pts = np.asarray(pts, dtype=LD).reshape(-1, 3)
    if origin is None:
        return pts
    xyz, rpy = origin
    (r, p, y) = (LD(a) for a in rpy)  # URDF rpy: fixed axes, R = Rz(yaw) Ry(pitch) Rx(roll), written out here (no code of the package)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]], dtype=LD)
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]], dtype=LD)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], dtype=LD)
    return pts @ (Rz @ Ry @ Rx).T + np.asarray(xyz, dtype=LD)[None]


def frame7(origin):
    xyz, rpy = origin
    return tuple(xyz) + tuple(quat_from_rpy(*rpy))


# ---- models -------------------------------------------------------------------------------------------------------------------------------------------------
def arm_with(points=None, radii=None, link=TIP):
    m = pr2_like()
    if points is not None:
        m.add_collision_points(link, points, radii)
    return m


def arm_with_box():
    m = pr2_like()
    m.add_collision_box(TIP, BOX)
    return m


def random_points(n, seed, scale=0.08):
    return np.random.default_rng(seed).uniform(-scale, scale, size=(n, 3))


O_BOX, O_SPH, O_MESH = ((0.02, -0.01, 0.03), (0.3, -0.2, 0.5)), ((0.05, 0.0, -0.02), (0.0, 0.4, 0.0)), ((-0.01, 0.02, 0.0), (-0.6, 0.1, 0.2))
MESH = np.array([[0.03, 0.0, 0.0], [-0.03, 0.01, 0.0], [0.0, 0.04, 0.01], [0.0, -0.04, 0.0], [0.005, 0.0, 0.05], [0.0, 0.0, -0.05], [0.01, 0.01, 0.01]])


def mixed_model():
    """box + sphere + mesh on one link, each with a non-identity origin"""
    m = pr2_like()
    m.add_collision_box(TIP, BOX, frame7(O_BOX))
    m.add_collision_sphere(TIP, 0.035, frame7(O_SPH))
    m.add_collision_points(TIP, MESH, None, frame7(O_MESH))
    return m


def mixed_expected():
    return np.vstack([expected_box(BOX, O_BOX), np.hstack([move([[0, 0, 0]], O_SPH), [[LD(0.035)]]]), np.hstack([move(MESH, O_MESH), np.zeros((len(MESH), 1), dtype=LD)])])


def function_cases():
    """name -> (model, group, goals): the shapes where the loop, the table offsets and the goal tables can go wrong"""
    out = {}
    P0, N0 = (0.55, -0.2, 0.7), (0.2, -0.3, 0.9)
    for n in (1, 2, 3, 5, 17, CAP):
        out["points_%d" % n] = (arm_with(random_points(n, n)), "right_arm", [TouchGoal(TIP, P0, N0)])
    # the minimum at the last / the first point for EVERY direction: one point with a radius that swallows the others; a tie: the same point twice
    small = random_points(9, 5, 0.01)
    out["min_is_last"] = (arm_with(np.vstack([small, [[0, 0, 0]]]), [0.0] * 9 + [0.5]), "right_arm", [TouchGoal(TIP, P0, N0)])
    out["min_is_first"] = (arm_with(np.vstack([[[0, 0, 0]], small]), [0.5] + [0.0] * 9), "right_arm", [TouchGoal(TIP, P0, N0)])
    out["tie"] = (arm_with(np.vstack([[[0, 0, 0]], small, [[0, 0, 0]]]), [0.5] + [0.0] * 9 + [0.5]), "right_arm", [TouchGoal(TIP, P0, N0)])
    m = pr2_like()
    m.add_collision_sphere(TIP, 0.05)
    out["sphere_only"] = (m, "right_arm", [TouchGoal(TIP, P0, N0)])
    out["box_sphere_mesh"] = (mixed_model(), "right_arm", [TouchGoal(TIP, P0, N0)])
    m = pr2_like()  # two goals on two links of a branching model (the arms behind the torso): the second goal's table starts behind the first's
    m.add_collision_points(TIP_L, random_points(6, 21))
    m.add_collision_box(TIP, BOX)
    m.add_collision_sphere("r_forearm_link", 0.07)  # (a link no goal names, in front of both in link order)
    out["two_links"] = (m, "all", [TouchGoal(TIP, P0, N0, weight=0.7), TouchGoal(TIP_L, (0.5, 0.3, 0.6), (0, 0, 1), weight=1.3)])
    out["beside_pose_goal"] = (arm_with_box(), "right_arm", [PoseGoal(TIP, (0.6, -0.2, 0.8), (0.1, 0.2, 0.3, 0.9)), TouchGoal(TIP, P0, N0)])
    sec = TouchGoal(TIP, (0.1, 0.2, 0.3), N0, weight=0.8)
    sec.secondary_ = True
    out["secondary"] = (arm_with_box(), "right_arm", [PositionGoal(TIP, (0.6, -0.2, 0.8)), sec])
    out["weight"] = (arm_with_box(), "right_arm", [TouchGoal(TIP, P0, N0, weight=0.37)])
    return out


# ---- costs and bounds ---------------------------------------------------------------------------------------------------------------------------------------
def costs_and_bounds(t, pr, params, frames, dp, dq, dist=None):
    """weighted cost (n, n_goals) in long double and its bound, for frames {link: (p, q)} known to dp / dq {link: (n,)}; `dist` (optional dict): per touch
    goal k the weighted |d| (n,) and its bound"""
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
            pts = t.model.collision_points(link)
            d = touch_distance(P, p, q, pts)
            c = d * d
            qn = np.linalg.norm(q64, axis=1)
            rot = 2 * d_q * (1 + qn * qn)
            dr = d_p * np.linalg.norm(P[3:6]) + (rot + C * U) * np.linalg.norm(pts[:, :3], axis=1).max() + C * U * (np.linalg.norm(P[:3]) + np.linalg.norm(p64, axis=1))
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


def sums(t, cost, bound):
    sec = np.array([g.isSecondary() for g in t.goals])
    out = []
    for mask in (~sec, sec):
        want = np.asarray(cost[:, mask].sum(axis=1), dtype=np.float64)
        out.append((want, bound[:, mask].sum(axis=1) + C * U * want))
    return out


def exact_frames(pr, seed, genes):
    R, p = pr.frames(seed, genes)
    return {l: (p[l], quat_from_rot_batch(R[l])) for l in set(pr.tips)}


def function_level(make_solver, name, stats, n=200):
    """bioik_eval_fitness in both FK modes and bioik_eval_check against the restatement; the worst error / bound ratios go to `stats`"""
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
    cost, bound = costs_and_bounds(t, pr, params, exact_frames(pr, seed, genes), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m})
    pa, sa = h.fitness(abi.FK_EXACT, seed, params, genes)
    for got, (want, bnd), what in zip((pa, sa), sums(t, cost, bound), ("exact primary", "exact secondary")):
        err = np.abs(got - want)
        r = stats.ratio(what, err, np.maximum(bnd, 1e-300), name)
        assert r <= 1.0, "%s: %s fitness off by %.3g, bound %.3g (row %d)" % (name, what, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))], int(np.argmax(err / np.maximum(bnd, 1e-300))))
    # the success test (problem.cpp:327-334, the default branch): weighted cost < min(dpos, dtwist)^2 for every primary goal; half of the rows get a plane
    # through their own lowest corner (a cost of nothing), and a decision may differ from the restatement's only inside the bound
    if all(g.opcode == abi.GOAL_TOUCH for g in goals if not g.isSecondary()):
        sp = abi.default_solve_params(dpos=-1.0, drot=-1.0, dtwist=1e-3)
        fr = exact_frames(pr, seed, genes)
        hits = 0
        rows = list(range(0, n, max(n // 16, 1)))
        for j, i in enumerate(rows):
            P1 = params.copy()
            for g, off in zip(t.goals, t.param_offsets):
                if not g.isSecondary() and j % 2 == 0:
                    link = model.link_index(g.link_name())
                    f1 = (fr[link][0][i:i + 1], fr[link][1][i:i + 1])
                    d = touch_distance(np.concatenate([np.zeros(3), P1[off + 3:off + 6]]), f1[0], f1[1], model.collision_points(link))
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
    # linearised phenotypes around a base: tip + sum of delta (gene - base), the quaternion not renormalised; frames and their bounds as
    # random_robot_cases.function_level builds them
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
    want, bnd = sums(t, cost, bound)[0]
    err = np.abs(pl - want)
    r = stats.ratio("linear primary", err, np.maximum(bnd, 1e-300), name)
    assert r <= 1.0, "%s: linearised primary fitness off by %.3g, bound %.3g" % (name, err.max(), bnd[np.argmax(err / np.maximum(bnd, 1e-300))])
    h.close()


def streamed(make_solver, device_arrays):
    """bioik_stream_fitness_device (genes [unit][D][pop]) gives the bits of bioik_eval_fitness, exact FK, on the same library"""
    model, group, goals = function_cases()["two_links"]
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
def refusals(make_solver, lib):
    import ctypes as Ct
    assert lib.bioik_goal_param_count(17) == 6 and lib.bioik_goal_param_count(18) == -1
    for model, code, word in ((arm_with(random_points(CAP + 1, 1)), abi.ERR_UNSUPPORTED, "BIOIK_MAX_TOUCH_POINTS"),
                              (pr2_like(), abi.ERR_INVALID_ARGUMENT, "no collision points"),
                              (arm_with(random_points(3, 1), link="r_forearm_link"), abi.ERR_INVALID_ARGUMENT, "no collision points"),
                              (cylinder_model(), abi.ERR_UNSUPPORTED, "cylinder"), (unresolved_mesh_model(), abi.ERR_UNSUPPORTED, "mesh without its vertices")):
        try:
            make_solver(ProblemTemplate(model, "right_arm", [TouchGoal(TIP, (0, 0, 0), (0, 0, 1))]))
        except solver.BioIKError as e:
            assert e.code == code and word in str(e) and word in lib.bioik_last_error().decode(), (code, str(e))
        else:
            raise AssertionError("accepted: " + word)
    m = unresolved_mesh_model()
    m.add_collision_points(TIP, MESH)  # the vertices supplied: accepted
    make_solver(ProblemTemplate(m, "right_arm", [TouchGoal(TIP, (0, 0, 0), (0, 0, 1))])).close()
    bad = arm_with_box().desc()
    bad_pts = np.array([[0.0, 0.0, 0.0, -0.5]])  # a negative radius that is not the marker: a malformed table, not "a cylinder"
    bad_first = np.zeros(arm_with_box().n_links + 1, dtype=np.int32)
    bad_first[1:] = 1
    bad.link_point_first, bad.link_points = abi.iptr(bad_first), abi.dptr(bad_pts)
    hm = Ct.c_void_p()
    assert lib.bioik_model_create(Ct.byref(bad), 0, Ct.byref(hm)) == abi.ERR_INVALID_ARGUMENT and "radius" in lib.bioik_last_error().decode()
    make_solver(ProblemTemplate(cylinder_model(), "right_arm", [PoseGoal(TIP)])).close()  # (the cylinder is refused only where a TouchGoal names its link)
    # a caller built against the header without link_point_first / link_points: the shorter struct_size creates a model (without points)
    m = arm_with_box()
    d = m.desc()
    d.struct_size = abi.ModelDesc.link_point_first.offset
    handle = Ct.c_void_p()
    assert lib.bioik_model_create(Ct.byref(d), 0, Ct.byref(handle)) == abi.OK, lib.bioik_last_error().decode()
    t = ProblemTemplate(m, "right_arm", [TouchGoal(TIP, (0, 0, 0), (0, 0, 1))])
    pd, prob = t.desc(), Ct.c_void_p()
    assert lib.bioik_problem_create(handle, Ct.byref(pd), Ct.byref(prob)) == abi.ERR_INVALID_ARGUMENT  # (that model has no points)
    lib.bioik_model_destroy(handle)
    d.struct_size = abi.ModelDesc.link_point_first.offset + 4
    assert lib.bioik_model_create(Ct.byref(d), 0, Ct.byref(handle)) == abi.ERR_INVALID_ARGUMENT


def unresolved_mesh_model():
    """a box and a <mesh> that is only named (as the URDF reader leaves it): scoring the box alone would be a silent approximation"""
    m = arm_with_box()
    m.link_meshes.setdefault(m.link_index(TIP), []).append(("package://x/pad.stl", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)))
    return m


def cylinder_model():
    m = pr2_like()
    m.add_collision_unsupported(TIP, "cylinder")
    return m


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------------------------
N_QUERIES = 16
SOLVE = dict(population=128, max_steps=64, islands=4, random_seed=5)  # (dtwist: the default, 1e-5)


def reachable_queries(t, h, n=N_QUERIES, seed=11):
    """per query: a random configuration inside the limits, its tip frame in long double, a random unit normal, and `position` at the box corner that is
    lowest along the normal -- the plane then touches the box at that configuration; the solve starts from another random configuration"""
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
    pts = np.asarray(m.collision_points(link), dtype=LD)
    params = np.zeros((n, t.param_count))
    for g, off in zip(t.goals, t.param_offsets):
        for i in range(n):
            corners = p[link][i][None] + pts[:, :3] @ R[link][i].T
            lowest = corners[np.argmin(corners @ np.asarray(normals[i], dtype=LD))]
            if g.opcode == abi.GOAL_TOUCH:
                params[i, off:off + 3], params[i, off + 3:off + 6] = np.asarray(lowest, dtype=np.float64), normals[i]
            else:  # the PositionGoal beside a secondary touch goal: the link's origin at the target
                params[i, off:off + 3] = np.asarray(p[link][i], dtype=np.float64)
    return seeds, params


def verify_solve(t, h, seeds, params, sol, fit, suc, min_success):
    """the asserts of a whole solve on the returned joint values, recomputed in long double.  Returns the number of successes."""
    pr = np_goals.Problem(t, h.active_variables, h.tip_links)
    n = sol.shape[0]
    won = 0
    for i in range(n):
        g1 = sol[i:i + 1, pr.active]
        b = rr.Bounds(pr, sol[i:i + 1].astype(np.float64))
        dist = {}
        cost, bound = costs_and_bounds(t, pr, params[i], exact_frames(pr, sol[i], g1), {l: b.dp(l) for l in b.m}, {l: b.dq(l) for l in b.m}, dist)
        prim = [k for k, g in enumerate(t.goals) if not g.isSecondary()]
        sec = [k for k, g in enumerate(t.goals) if g.isSecondary()]
        assert np.array_equal(sol[i, np.setdiff1d(np.arange(h.V), pr.active)], seeds[i, np.setdiff1d(np.arange(h.V), pr.active)])
        # success: the weighted |d| of every primary touch goal below dtwist = 1e-5 (problem.cpp:327-334: weighted cost < dtwist^2), within the bound of its
        # recomputation; a query that is not flagged has a primary goal that is not below it
        touch = [k for k in prim if k in dist]
        if suc[i]:
            for k in touch:
                assert dist[k][0][0] < 1e-5 + dist[k][1][0], (i, k, dist[k])
        elif len(touch) == len(prim):
            assert any(dist[k][0][0] >= 1e-5 - dist[k][1][0] for k in touch), (i, dist)
        want = float(cost[0, prim].sum()) + (float(cost[0, sec].sum()) if suc[i] else 0.0)
        bnd = bound[0, prim].sum() + (bound[0, sec].sum() if suc[i] else 0.0) + C * U * want
        assert abs(fit[i] - want) <= bnd, (i, fit[i], want, bnd)
        won += int(suc[i])
    assert won >= min_success, "%d of %d queries solved" % (won, n)
    return won


def solve_template(variant):
    m = arm_with_box()
    if variant == "secondary":
        sec = TouchGoal(TIP, (0, 0, 0), (0, 0, 1))
        sec.secondary_ = True
        return ProblemTemplate(m, "right_arm", [PositionGoal(TIP), sec])
    return ProblemTemplate(m, "right_arm", [TouchGoal(TIP, (0, 0, 0), (0, 0, 1))])


def whole_solve(make_solver, variant="primary"):
    """variant: primary | secondary (beside a PositionGoal) | gd | ranked (bioik_solve_batch_ranked, k = 2).  Returns (solver, results) for bit comparisons."""
    t = solve_template(variant)
    h = make_solver(t)
    seeds, params = reachable_queries(t, h)
    if variant == "gd":
        p = abi.default_solve_params(mode="gd", max_steps=64, islands=4, random_seed=5)
    else:
        p = abi.default_solve_params(**SOLVE)
    if variant == "ranked":
        sol, fit, suc, steps, count = h.solve_batch_ranked(p, seeds, params, 2, 0.0)
        assert count.min() >= 1
        best = h.solve_batch(p, seeds, params)
        assert all(np.array_equal(a[:, 0], b) for a, b in zip((sol, fit, suc, steps), best))  # row 0: the plain answer
        for r in range(2):
            rows = count > r
            verify_solve(t, h, seeds[rows], params[rows], sol[rows, r], fit[rows, r], suc[rows, r], N_QUERIES // 2 if r == 0 else 0)
        res = (sol, fit, suc, steps, count)
    else:
        res = h.solve_batch(p, seeds, params)
        verify_solve(t, h, seeds, params, res[0], res[1], res[2], N_QUERIES // 2)
    return h, t, seeds, params, p, res


MAPPINGS = [
    {"BIOIK_SOLVE_THREADS": "64"}, {"BIOIK_SOLVE_THREADS": "128"}, {"BIOIK_SOLVE_THREADS": "256"},
    {"BIOIK_SOLVE_THREADS": "256", "BIOIK_SOLVE_SPECIES_PARALLEL": "0"},
    {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_STORE_CHILDREN": "0"}, {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_STORE_CHILDREN": "0"},
    {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_CHILD_PAIRS": "0"}, {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_GENERAL": "1"},
    {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_SPECIES_PARALLEL": "1"},
    {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_SPECIES_PARALLEL": "1", "BIOIK_SOLVE_STORE_CHILDREN": "0"},
    {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_COLUMNLESS": "1"}, {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_COLUMNLESS": "1"},
    {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_COLUMNLESS": "2"},
    {"BIOIK_SOLVE_THREADS": "64", "BIOIK_SOLVE_SPECIES_PARALLEL": "1", "BIOIK_SOLVE_COLUMNLESS": "2"},
    {"BIOIK_SOLVE_THREADS": "256", "BIOIK_SOLVE_COLUMNLESS": "1"},
    {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_COLUMNLESS": "0", "BIOIK_SOLVE_STORE_CHILDREN": "0"},
    {"BIOIK_SOLVE_TWO_PHASE": "1"}, {"BIOIK_SOLVE_TWO_PHASE": "2", "BIOIK_SOLVE_THREADS": "256"}, {"BIOIK_SOLVE_TWO_PHASE": "1", "BIOIK_SOLVE_GENERAL": "1"},
    {"BIOIK_SOLVE_TWO_PHASE": "1,2,4"}, {"BIOIK_SOLVE_FUSED_SELECT": "0"}, {"BIOIK_SOLVE_PRESELECT": "0"},
]


def mapping_independence(make_solver, monkeypatch, variants=("primary", "secondary"), steps=SOLVE["max_steps"], n=N_QUERIES, islands=SOLVE["islands"]):
    """the whole-solve case (16 queries, 64 steps, four islands by default) gives the same bits under every lane mapping the BIOIK_SOLVE_* switches can
    force for it (a problem with a TouchGoal runs in the general kernel flavour: the switches that name a lean mapping are passed over by the launcher)"""
    for variant in variants:
        t = solve_template(variant)
        h = make_solver(t)
        seeds, params = reachable_queries(t, h, n)
        for fk in (abi.FK_EXACT, abi.FK_LINEAR):
            p = abi.default_solve_params(population=128, max_steps=steps, islands=islands, random_seed=5, fk_mode=fk)
            base = h.solve_batch(p, seeds, params)
            for env in MAPPINGS:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                got = h.solve_batch(p, seeds, params)
                for k in env:
                    monkeypatch.delenv(k)
                assert all(np.array_equal(a, b) for a, b in zip(base, got)), (variant, fk, env)
        h.close()
