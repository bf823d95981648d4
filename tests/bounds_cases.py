"""Per-query variable bounds (bioik_solve_batch_bounded, include/bioik_hip.h: PER-QUERY VARIABLE BOUNDS), shared by the host-simulator suite
(tests/test_hostsim_bounds.py) and the GPU suite (tests/test_gpu_bounds.py).

The rule is "a query with a row of bounds is solved as if the model had been created with them", so the reference of a whole solve is the oracle on a NARROWED
MODEL: per query a copy of the robot with var_min / var_max / var_bounded edited, one oracle solve of that one row under its first_query index.  The rule itself
is checked in isolation (bioik_eval_bounds against `restate`, written from the header's text), the entry points by identities, the windows by a property.
Doubles are compared by bit pattern: a pinned variable under a limit goal may give costs that are no numbers.

`ctx` is the suite's context (migration_cases.Ctx): make_solver(template) (the library under test), make_sim(template) (the host simulator), dev (device arrays,
streams, captures), mp (monkeypatch), report (limit_cases.Report)."""
import copy

import numpy as np

import limit_cases as lc
from bio_ik_amd import AvoidJointLimitsGoal, CenterJointsGoal, JointVariableGoal, PoseGoal, ProblemTemplate, abi
from bio_ik_amd.solver import BioIKError
from bio_ik_amd.workload import make_queries
from conftest import gnarly_robot, mimic_robot
from oracle import orc

NAMES = ("solutions", "fitness", "success", "steps")
DBL_MAX = np.finfo(np.float64).max
FLT_MAX = float(np.finfo(np.float32).max)
FULL_TURN = 2 * np.pi * 0.9999  # (robot_info.h:82-84)
N = 6  # queries of every solve here; population 16, 9 steps, random_seed 3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what):
    for name, x, y in zip(NAMES, got, want):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), "%s: %s differ" % (what, name)


def params(**kw):
    return abi.default_solve_params(**dict(dict(population=16, max_steps=9, random_seed=3), **kw))


# ---- the problems ------------------------------------------------------------------------------------------------------------------------------------------
def _secondary(g):
    g.secondary_ = True
    return g


# name -> (model, group, goals): a template and, from the same three, the template of a narrowed copy of the model
RECIPES = {
    "arm": (lambda pr2: pr2, "right_arm", lambda: [PoseGoal("r_wrist_roll_link")]),
    "mimic": (lambda pr2: mimic_robot(), "arm", lambda: [PoseGoal("tool")]),  # ops that are no genes
    "jv": (lambda pr2: pr2, "right_arm", lambda: [PoseGoal("r_wrist_roll_link"), JointVariableGoal("r_elbow_flex_joint", -1.0, weight=0.5)]),  # genes do not follow ops
    "arm_avoid": (lambda pr2: pr2, "right_arm", lambda: [PoseGoal("r_wrist_roll_link"), AvoidJointLimitsGoal(0.5)]),
    "arm_center_sec": (lambda pr2: pr2, "right_arm", lambda: [PoseGoal("r_wrist_roll_link"), _secondary(CenterJointsGoal(0.5))]),
    "gnarly": (lambda pr2: gnarly_robot(), "body", lambda: [PoseGoal("a_tool")]),  # a prismatic joint inside the chain (the rule's cases only)
}
_models, _templates = {}, {}


def model_of(name, pr2):
    if name not in _models:
        _models[name] = RECIPES[name][0](pr2)
    return _models[name]


def template(name, pr2):
    if name not in _templates:
        _templates[name] = ProblemTemplate(model_of(name, pr2), RECIPES[name][1], RECIPES[name][2]())
    return _templates[name]


def narrowed_template(name, pr2, act, lo_row, hi_row):
    """the template on a copy of the model whose active variables with a valid pair of bounds have them as var_min / var_max, var_bounded = 1"""
    m = copy.deepcopy(model_of(name, pr2))
    for v in act:
        if np.isfinite(lo_row[v]) and np.isfinite(hi_row[v]) and lo_row[v] <= hi_row[v]:
            m.var_min[v], m.var_max[v], m.var_bounded[v] = float(lo_row[v]), float(hi_row[v]), 1
    m._keep = None  # (arrays() caches)
    return ProblemTemplate(m, RECIPES[name][1], RECIPES[name][2]())


def queries(t, h):
    return make_queries(t, h.active_variables, h.fk_genes, N, seed=5, kind="tracking", noise=0.05)[:2]


def windows(model, act, seeds, below, above):
    """[seed - below, seed + above] on the active variables, cut to the model's limits wherever those are finite; NaN elsewhere"""
    lo, hi = np.full(seeds.shape, np.nan), np.full(seeds.shape, np.nan)
    vmin, vmax = np.asarray(model.var_min, dtype=np.float64), np.asarray(model.var_max, dtype=np.float64)
    for v in act:
        lo[:, v], hi[:, v] = seeds[:, v] - below, seeds[:, v] + above
        if np.isfinite(vmin[v]):
            lo[:, v] = np.maximum(lo[:, v], vmin[v])
        if np.isfinite(vmax[v]):
            hi[:, v] = np.minimum(hi[:, v], vmax[v])
    return lo, hi


def revolute_variables(model):
    k = model.arrays()
    out = np.zeros(model.n_variables, dtype=bool)
    for l in range(len(k["joint_type"])):
        if k["joint_type"][l] == abi.JOINT_REVOLUTE and k["joint_first_variable"][l] >= 0:
            out[k["joint_first_variable"][l]] = True
    return out


def mixed_bounds(model, act, seeds):
    """the five kinds of bounds, one per query, and an all-NaN row: [0] seed +- 0.2 cut to the model; [1] seed +- 0.02; [2] [seed + 0.05, seed + 0.3]: the
    seed lies outside; [3] lo == hi == seed on one variable, nothing on the others; [4] a +- 3.2 window on a revolute variable (a full turn: it loses
    its clip), nothing on the others; [5] no bounds"""
    assert seeds.shape[0] == N
    lo, hi = np.full(seeds.shape, np.nan), np.full(seeds.shape, np.nan)
    a, b = windows(model, act, seeds, 0.2, 0.2)
    lo[0], hi[0] = a[0], b[0]
    a, b = windows(model, act, seeds, 0.02, 0.02)
    lo[1], hi[1] = a[1], b[1]
    for v in act:
        lo[2, v], hi[2, v] = seeds[2, v] + 0.05, seeds[2, v] + 0.3
    pin = int(act[len(act) // 2])
    lo[3, pin] = hi[3, pin] = seeds[3, pin]
    rev = [int(v) for v in act if revolute_variables(model)[v]]
    lo[4, rev[-1]], hi[4, rev[-1]] = seeds[4, rev[-1]] - 3.2, seeds[4, rev[-1]] + 3.2
    return lo, hi


# ---- 1: the rule in isolation --------------------------------------------------------------------------------------------------------------------------------
def restate(info, revolute, op_var, op_gene, lo, hi):
    """the header's rule on rows lo, hi [n][V] -> [n][ops][6] = vmin, vmax, span, clip_min, clip_max, unbounded.  info: the oracle's robot_info() of the model
    ([V]: clip_min, clip_max, span, min, max, .)"""
    out = np.zeros((lo.shape[0], max(len(op_var), 1), 6))
    for q in range(lo.shape[0]):
        for k, (v, g) in enumerate(zip(op_var, op_gene)):
            cmin, cmax, span, vmin, vmax = info[v, :5]
            a, b = lo[q, v], hi[q, v]
            if g >= 0 and np.isfinite(a) and np.isfinite(b) and a <= b:
                bounded = not (revolute[v] and b - a >= FULL_TURN)
                vmin, vmax = a, b
                cmin, cmax = (a, b) if bounded else (-DBL_MAX, DBL_MAX)
                span = b - a
                if not (span >= 0 and span < FLT_MAX):
                    span = 1.0
            out[q, k] = (vmin, vmax, span, cmin, cmax, 1.0 if cmax == DBL_MAX else 0.0)
    return out


def rule_rows(V):
    """rows of bounds, every variable treated alike in a row"""
    under_flt = float(np.nextafter(FLT_MAX, 0.0))
    rows = [
        (np.nan, np.nan), (np.nan, 0.5), (-0.5, np.nan), (-np.inf, 0.5), (-0.5, np.inf), (-np.inf, np.inf), (0.5, -0.5),  # keep the model's
        (0.25, 0.25), (-0.5, 0.5), (-0.0, 0.0),  # lo == hi, an ordinary window, zeros of both signs
        (-FLT_MAX / 2, FLT_MAX / 2), (-1e300, 1e300), (0.0, under_flt),  # a span of FLT_MAX, above, just under
        (0.0, float(np.nextafter(FULL_TURN, 0.0))), (0.0, FULL_TURN), (-3.2, 3.2),  # revolute: just under the full turn, at it, beyond
    ]
    lo = np.array([[a] * V for a, _ in rows], dtype=np.float64)
    hi = np.array([[b] * V for _, b in rows], dtype=np.float64)
    return lo, hi


def b1_rule(ctx, pr2, name):
    t = template(name, pr2)
    h = ctx.make_solver(t)
    o = orc.Oracle(t)
    op_var, op_gene = h.op_variables()
    assert len(op_var) == h.n_ops() and sorted(op_gene[op_gene >= 0]) == list(range(h.D))
    assert np.array_equal(np.asarray(h.active_variables)[op_gene[op_gene >= 0]], op_var[op_gene >= 0])
    if name == "mimic":
        assert (op_gene < 0).any(), "precondition: ops that are no genes"
    revolute = revolute_variables(t.model)
    if name == "gnarly":
        assert any(not revolute[v] for v in h.active_variables), "precondition: an active prismatic variable"
    info = o.robot_info()
    lo, hi = rule_rows(h.V)
    rng = np.random.default_rng(7)  # ... and a row with another pair per variable, NaNs among them
    lo = np.vstack([lo, rng.uniform(-1.0, 0.0, h.V)[None, :]])
    hi = np.vstack([hi, rng.uniform(0.0, 1.0, h.V)[None, :]])
    lo[-1, ::3] = np.nan
    want = restate(info, revolute, op_var, op_gene, lo, hi)
    got = h.eval_bounds(lo, hi)
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), "bioik_eval_bounds differs from the restated rule at (row, op, column) %s" % np.argwhere(bits(got) != bits(want))[:8].tolist()
    # an all-NaN row is what the oracle's robot_info() reports for the model, bit for bit
    for k, v in enumerate(op_var):
        assert np.array_equal(bits(got[0, k, :5]), bits(info[v, [3, 4, 2, 0, 1]])), (k, v)
    # (the rows are what their comments say)
    gene_ops = np.nonzero(op_gene >= 0)[0]
    assert np.array_equal(bits(got[:7]), bits(np.repeat(got[:1], 7, axis=0))), "rows that keep the model's bounds"
    assert (got[7, gene_ops, 2] == 0.0).all() and (got[10, gene_ops, 2] == 1.0).all() and (got[11, gene_ops, 2] == 1.0).all() and (got[12, gene_ops, 2] == under_flt_span()).all()
    rev_ops = [k for k in gene_ops if revolute[op_var[k]]]
    other_ops = [k for k in gene_ops if not revolute[op_var[k]]]
    assert rev_ops and (got[13, rev_ops, 5] == 0.0).all() and (got[14, rev_ops, 5] == 1.0).all() and (got[15, rev_ops, 5] == 1.0).all()
    assert (got[14, other_ops, 5] == 0.0).all()
    # entries of variables that are no active variables are not read
    lo2, hi2 = lo.copy(), hi.copy()
    inactive = np.setdiff1d(np.arange(h.V), np.asarray(h.active_variables))
    lo2[:, inactive], hi2[:, inactive] = -7.0, 7.0
    assert np.array_equal(bits(h.eval_bounds(lo2, hi2)), bits(got))
    h.close(), o.close()


def under_flt_span():
    return float(np.nextafter(FLT_MAX, 0.0))


# ---- 2: as if the model had these bounds -------------------------------------------------------------------------------------------------------------------
# (template, mode, fk_mode, islands): every mode, both fk_modes for the bio2 family, 1 and 3 islands on the arm; the other templates under bio2_memetic (and one
# point solver on the mimic robot)
SOLVES = {}
for _mode in ("bio2", "bio2_memetic", "bio2_memetic_l", "gd", "gd_r", "gd_c", "jac"):
    for _isl in (1, 3):
        SOLVES["arm-%s-exact-i%d" % (_mode, _isl)] = ("arm", _mode, abi.FK_EXACT, _isl)
for _mode in ("bio2", "bio2_memetic", "bio2_memetic_l"):
    SOLVES["arm-%s-linear-i1" % _mode] = ("arm", _mode, abi.FK_LINEAR, 1)
SOLVES["arm-bio2_memetic-linear-i3"] = ("arm", "bio2_memetic", abi.FK_LINEAR, 3)
for _name in ("mimic", "jv", "arm_avoid", "arm_center_sec"):
    for _isl in (1, 3):
        SOLVES["%s-bio2_memetic-exact-i%d" % (_name, _isl)] = (_name, "bio2_memetic", abi.FK_EXACT, _isl)
SOLVES["mimic-jac-exact-i3"] = ("mimic", "jac", abi.FK_EXACT, 3)
SOLVES["arm_avoid-gd_r-exact-i3"] = ("arm_avoid", "gd_r", abi.FK_EXACT, 3)
_inputs, _oracle_results, _sim_results = {}, {}, {}


def solve_params(case):
    name, mode, fk, islands = SOLVES[case]
    return params(mode=mode, fk_mode=fk, islands=islands)


def inputs(ctx, pr2, name):
    """seeds, goal parameters and the mixed bounds of a template: made once, shared, never changed"""
    if name not in _inputs:
        t = template(name, pr2)
        h = ctx.make_sim(t)
        seeds, gp = queries(t, h)
        lo, hi = mixed_bounds(t.model, np.asarray(h.active_variables), seeds)
        _inputs[name] = tuple(np.ascontiguousarray(x) for x in (seeds, gp, lo, hi))
        for x in _inputs[name]:
            x.setflags(write=False)
        h.close()
    return _inputs[name]


def oracle_rows(ctx, pr2, case):
    """per query the oracle on the narrowed model, that one row under its first_query index: computed once per case"""
    if case not in _oracle_results:
        name = SOLVES[case][0]
        seeds, gp, lo, hi = inputs(ctx, pr2, name)
        p = solve_params(case)
        rows = []
        act = None
        for q in range(N):
            if act is None:
                o0 = orc.Oracle(template(name, pr2))
                act = np.asarray(o0.active_variables).copy()
                o0.close()
            o = orc.Oracle(narrowed_template(name, pr2, act, lo[q], hi[q]))
            rows.append(o.solve_batch(p, orc.RNG_COUNTER, seeds[q:q + 1], gp[q:q + 1], first_query_index=q))
            o.close()
        _oracle_results[case] = tuple(np.concatenate([r[i] for r in rows]) for i in range(4))
        for x in _oracle_results[case]:
            x.setflags(write=False)
    return _oracle_results[case]


def b2_as_if(ctx, pr2, case):
    name = SOLVES[case][0]
    seeds, gp, lo, hi = inputs(ctx, pr2, name)
    p = solve_params(case)
    h = ctx.make_solver(template(name, pr2))
    ctx.report.read()
    got = h.solve_batch(p, seeds, gp, bounds=(lo, hi))
    k = [x for x in ctx.report.kernels(ctx.report.read()) if x.startswith("k_solve")]
    assert k and set(k) == {"k_solve_bounded" if p.mode in (abi.MODE_BIO2, abi.MODE_BIO2_MEMETIC, abi.MODE_BIO2_MEMETIC_L) else "k_solve_point_bounded"}, k
    same(got, oracle_rows(ctx, pr2, case), case + " against the oracle on the narrowed models")
    plain = h.solve_batch(p, seeds, gp)
    same([x[N - 1:] for x in got], [x[N - 1:] for x in plain], case + ": the all-NaN row against the plain call's")
    if ctx.make_sim is not ctx.make_solver:  # the library under test against the host simulator of the same kernel bodies
        if case not in _sim_results:
            s = ctx.make_sim(template(name, pr2))
            _sim_results[case] = s.solve_batch(p, seeds, gp, bounds=(lo, hi))
            s.close()
        same(got, _sim_results[case], case + " against the host simulator")
    h.close()
    return got


def b2_table_is_what_the_issue_measured(ctx, pr2):
    """the figures the oracle gave on narrowed models (the issue's table), on the library under test: what the cases above compare is not vacuous"""
    seeds, gp, lo, hi = inputs(ctx, pr2, "arm")
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    act = np.asarray(h.active_variables)
    p = params()
    a, b = windows(t.model, act, seeds, 0.2, 0.2)
    sol, fit, suc, steps = h.solve_batch(p, seeds, gp, bounds=(a, b))
    assert suc.all() and steps.min() >= 4 and steps.max() <= 6, (suc, steps)
    a, b = windows(t.model, act, seeds, 0.02, 0.02)
    sol, fit, suc, steps = h.solve_batch(p, seeds, gp, bounds=(a, b))
    assert not suc.any() and ((sol[:, act] >= a[:, act]) & (sol[:, act] <= b[:, act])).all()
    a, b = np.full(seeds.shape, np.nan), np.full(seeds.shape, np.nan)
    a[:, act], b[:, act] = seeds[:, act] + 0.05, seeds[:, act] + 0.3
    sol, fit, suc, steps = h.solve_batch(p, seeds, gp, bounds=(a, b))
    returned_seed = [bool(np.array_equal(sol[q], seeds[q])) for q in range(N)]
    assert not suc.any() and sum(returned_seed) == 4, (suc, returned_seed)  # (the solver does not clip the seed)
    sol, fit, suc, steps = h.solve_batch(params(mode="jac"), seeds, gp, bounds=windows(t.model, act, seeds, 0.2, 0.2))
    assert suc.all()
    h.close()


# ---- 3: identities -----------------------------------------------------------------------------------------------------------------------------------------
def b3_no_bounds_is_the_plain_call(ctx, pr2):
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp, lo, hi = inputs(ctx, pr2, "arm")
    for kw in (dict(), dict(islands=3), dict(mode="jac"), dict(schedule=abi.SCHEDULE_THROUGHPUT)):
        ctx.report.read()
        want = h.solve_batch(params(**kw), seeds, gp)
        k_want = ctx.report.kernels(ctx.report.read())
        got = h.solve_batch(params(**kw), seeds, gp, bounds=(None, None))  # (bioik_solve_batch_bounded with both pointers null)
        k_got = ctx.report.kernels(ctx.report.read())
        same(got, want, "both arrays null %s" % kw)
        assert k_want and k_got == k_want and not any("bounded" in x for x in k_got), (k_want, k_got)
    h.close()


def device_call(ctx, h, p, seeds, gp, lo, hi, stream_index=2):
    b = ctx.dev.buf
    ins = [b(np.array(x, copy=True)) for x in (seeds, gp, lo, hi)]
    n = seeds.shape[0]
    outs = (b(np.zeros((n, h.V))), b(np.zeros(n)), b(np.zeros(n, dtype=np.int32)), b(np.zeros(n, dtype=np.int32)))
    s = ctx.dev.stream(stream_index)

    def enqueue():
        with ctx.dev.on(s):
            h.solve_batch_device(p, n, ins[0].ptr, ins[1].ptr, *[o.ptr for o in outs], ctx.dev.handle(s), bounds=(ins[2].ptr, ins[3].ptr))

    return s, enqueue, ins, outs


def b3_three_forms(ctx, pr2):
    """host, submit / wait and device forms agree; a sharded call with set_first_query equals the unsharded one"""
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp, lo, hi = inputs(ctx, pr2, "arm")
    for kw in (dict(), dict(islands=3), dict(mode="gd_r", islands=3)):
        p = params(**kw)
        want = h.solve_batch(p, seeds, gp, bounds=(lo, hi))
        tickets = [h.submit_batch(p, seeds, gp, bounds=(lo, hi)) for _ in range(2)]  # (two in flight on one handle)
        for tk in tickets:
            same(h.wait_batch(tk), want, "submit / wait %s" % kw)
        s, enqueue, ins, outs = device_call(ctx, h, p, seeds, gp, lo, hi)
        enqueue()
        ctx.dev.sync()
        same(tuple(o.get() for o in outs), want, "the device form %s" % kw)
        parts = []
        for a, b in ((0, 2), (2, N)):
            h.set_first_query(a)
            parts.append(h.solve_batch(p, seeds[a:b], gp[a:b], bounds=(lo[a:b], hi[a:b])))
        h.set_first_query(0)
        same(tuple(np.concatenate([x[i] for x in parts]) for i in range(4)), want, "two shards with set_first_query %s" % kw)
    h.close()


def b3_plans(ctx, pr2):
    """island_migration = 3 with 3 islands against the simulator; a hand-over forced by BIOIK_SOLVE_TWO_PHASE equals the one-launch call; under the throughput
    schedule the call runs as under the latency schedule"""
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp, lo, hi = inputs(ctx, pr2, "arm")
    p = params(islands=3, island_migration=3)
    ctx.report.read()
    got = h.solve_batch(p, seeds, gp, bounds=(lo, hi))
    k = ctx.report.kernels(ctx.report.read())
    assert k.count("k_migrate_mark") == 2 and k.count("k_solve_bounded") == 3 and [x for x in k if x.startswith("k_solve")] == ["k_solve_bounded"] * 3, k
    s = ctx.make_sim(t)
    same(got, s.solve_batch(p, seeds, gp, bounds=(lo, hi)), "island_migration = 3, 3 islands, against the host simulator")
    s.close()
    off = h.solve_batch(params(islands=3), seeds, gp, bounds=(lo, hi))
    assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(got, off)), "precondition: the migration changes a result"
    for kw in (dict(), dict(islands=3)):
        one = h.solve_batch(params(**kw), seeds, gp, bounds=(lo, hi))
        with ctx.env(BIOIK_SOLVE_TWO_PHASE="2,5"):
            ctx.report.read()
            two = h.solve_batch(params(**kw), seeds, gp, bounds=(lo, hi))
            k = [x for x in ctx.report.kernels(ctx.report.read()) if x.startswith("k_solve")]
        assert k == ["k_solve_bounded"] * 3, k
        same(two, one, "hand-overs after steps 2 and 5 %s" % kw)
        ctx.report.read()
        thr = h.solve_batch(params(schedule=abi.SCHEDULE_THROUGHPUT, **kw), seeds, gp, bounds=(lo, hi))
        assert set(x for x in ctx.report.kernels(ctx.report.read()) if x.startswith("k_solve")) == {"k_solve_bounded"}
        same(thr, one, "the throughput schedule %s" % kw)
    h.close()


def b3_capture(ctx, pr2):
    """one capture and two replays of the device form equal the eager call (the second replay on new bounds)"""
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp, lo, hi = inputs(ctx, pr2, "arm")
    for kw in (dict(islands=3), dict()):
        p = params(**kw)
        want = h.solve_batch(p, seeds, gp, bounds=(lo, hi))
        s, enqueue, ins, outs = device_call(ctx, h, p, seeds, gp, lo, hi, stream_index=4)
        enqueue()  # (the one eager call of the same plan)
        ctx.dev.sync()
        same(tuple(o.get() for o in outs), want, "eager %s" % kw)
        g = ctx.dev.capture(s, enqueue)
        for replay in range(2):
            for o in outs:
                o.zero()
            ctx.dev.replay(g)
            ctx.dev.sync()
            same(tuple(o.get() for o in outs), want, "replay %d %s" % (replay, kw))
        ctx.dev.destroy(g)
    h.close()


# ---- 4: property -------------------------------------------------------------------------------------------------------------------------------------------
def b4_inside(ctx, pr2):
    """seeds inside their windows: every returned active variable lies inside [lo, hi], successes and failures alike"""
    n_fail = n_ok = 0
    for name, kw in (("arm", dict()), ("arm", dict(islands=3)), ("arm", dict(mode="gd_r", islands=3)), ("arm", dict(mode="jac")), ("mimic", dict()), ("arm_avoid", dict())):
        t = template(name, pr2)
        h = ctx.make_solver(t)
        seeds, gp = inputs(ctx, pr2, name)[:2]
        act = np.asarray(h.active_variables)
        for c in (0.2, 0.02, 0.0):
            lo, hi = windows(t.model, act, seeds, c, c)
            assert ((seeds[:, act] >= lo[:, act]) & (seeds[:, act] <= hi[:, act])).all(), "precondition: the seeds lie inside"
            sol, fit, suc, steps = h.solve_batch(params(**kw), seeds, gp, bounds=(lo, hi))
            assert ((sol[:, act] >= lo[:, act]) & (sol[:, act] <= hi[:, act])).all(), (name, kw, c)
            n_ok, n_fail = n_ok + int(suc.sum()), n_fail + int((suc == 0).sum())
        h.close()
    assert n_ok and n_fail, "precondition: successes and failures alike"


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------------------------------
def code(call):
    try:
        call()
        return abi.OK
    except BioIKError as e:
        assert str(e)
        return e.code


def b5_one_null(ctx, pr2):
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp, lo, hi = inputs(ctx, pr2, "arm")
    ctx.report.read()
    for bounds in ((lo, None), (None, hi)):
        for call in (lambda: h.solve_batch(params(), seeds, gp, bounds=bounds), lambda: h.submit_batch(params(), seeds, gp, bounds=bounds)):
            assert code(call) == abi.ERR_INVALID_ARGUMENT
    # ... the outputs untouched, through the entry itself
    import ctypes as C
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    sol, fit = np.full((N, h.V), 7.0), np.full(N, 7.0)
    suc, steps = np.full(N, 7, dtype=np.int32), np.full(N, 7, dtype=np.int32)
    rc = h.L.bioik_solve_batch_bounded(h.problem, C.byref(params()), N, seeds.ctypes.data_as(pd), gp.ctypes.data_as(pd), lo.ctypes.data_as(pd), None,
                                       sol.ctypes.data_as(pd), fit.ctypes.data_as(pd), suc.ctypes.data_as(pi), steps.ctypes.data_as(pi))
    assert rc == abi.ERR_INVALID_ARGUMENT and (sol == 7.0).all() and (fit == 7.0).all() and (suc == 7).all() and (steps == 7).all()
    s, enqueue, ins, outs = device_call(ctx, h, params(), seeds, gp, lo, hi)
    assert code(lambda: h.solve_batch_device(params(), N, ins[0].ptr, ins[1].ptr, *[o.ptr for o in outs], ctx.dev.handle(s), bounds=(ins[2].ptr, None))) == abi.ERR_INVALID_ARGUMENT
    assert not ctx.report.kernels(ctx.report.read()), "nothing launched"
    assert h.L.bioik_eval_bounds(h.problem, 1, None, hi.ctypes.data_as(pd), fit.ctypes.data_as(pd)) == abi.ERR_INVALID_ARGUMENT
    assert h.L.bioik_eval_bounds(h.problem, 0, None, None, None) == abi.OK
    h.close()


def solve_lds(n_ops, V, P, T, bounded):
    """bytes of LDS of k_solve / k_solve_bounded for a problem without parked frames and without secondary goals, exact FK, 16 children per species on fewer
    than 32 genes (64 lanes, a species group per half wavefront, one genotype column per lane): make_layout (bio_ik_amd/csrc/bioik_kernels.h) restated; the
    bounded layout holds 6 m instead of 2 m doubles of bounds"""
    m, lanes, groups = max(n_ops, 1), 64, 2
    o = V + max(P, 1) + 16 * m + m + 8 + 24 + (6 if bounded else 2) * m + m * lanes
    g = 9 * m
    g += g & 1
    if not 32 * max(T, 1) <= 4 * m:
        g += 32 * max(T, 1)
    g += 7 * T + 7 * T * m + m
    g += 4 * (lanes // 64) + 4 + 4
    return (o + g * groups) * 8


def b5_lds_edge(ctx, pr2):
    """a problem at the edge of a CU's LDS (limit_cases.centipede under a BalanceGoal: n ops, a tip per massive link, 7 T m doubles of linear model per species
    group): the plain call runs, the bounded one -- 32 m bytes more -- is refused with BIOIK_ERR_UNSUPPORTED, nothing launched"""
    import re
    from bio_ik_amd import BalanceGoal
    found = None
    for n in range(8, 32):
        for T in range(n + 1, 65):
            if solve_lds(n, n, 14, T, False) <= lc.LDS_CU < solve_lds(n, n, 14, T, True):
                found = (n, T)
                break
        if found:
            break
    assert found, "no problem size at the edge"
    n, T = found
    m = lc.centipede(n, T - n)
    t = ProblemTemplate(m, "body", [PoseGoal("seg%d" % (n - 1)), BalanceGoal()])
    h = ctx.make_solver(t)
    assert (h.n_ops(), h.V, h.P, h.T) == (n, n, 14, T)
    seeds = np.zeros((1, h.V))
    gp = np.ascontiguousarray(t.pack_params()).reshape(1, -1)
    p = abi.default_solve_params(population=16, max_steps=1, random_seed=1)
    ctx.report.read()
    sol, fit, suc, steps = h.solve_batch(p, seeds, gp)
    text = ctx.report.read()
    assert ctx.report.kernels(text) == ["k_solve"] and steps[0] == 1
    assert int(re.findall(r"LDS (\d+) B", text)[-1]) == solve_lds(n, n, 14, T, False), "the restated layout is the launcher's"
    lo, hi = np.full(seeds.shape, np.nan), np.full(seeds.shape, np.nan)
    assert code(lambda: h.solve_batch(p, seeds, gp, bounds=(lo, hi))) == abi.ERR_UNSUPPORTED
    assert not ctx.report.kernels(ctx.report.read()), "nothing launched"
    h.close()
    # ... and with one tip less the bounded layout fits again: far beyond 64 KiB (the launch needs its explicit allowance), all-NaN rows give the plain call's bits
    assert 64 * lc.KIB < solve_lds(n, n, 14, T - 1, True) <= lc.LDS_CU
    t = ProblemTemplate(lc.centipede(n, T - 1 - n), "body", [PoseGoal("seg%d" % (n - 1)), BalanceGoal()])
    h = ctx.make_solver(t)
    seeds = np.zeros((1, h.V))
    gp = np.ascontiguousarray(t.pack_params()).reshape(1, -1)
    lo, hi = np.full(seeds.shape, np.nan), np.full(seeds.shape, np.nan)
    ctx.report.read()
    got = h.solve_batch(p, seeds, gp, bounds=(lo, hi))
    assert ctx.report.kernels(ctx.report.read()) == ["k_solve_bounded"]
    same(got, h.solve_batch(p, seeds, gp), "at the edge, inside")
    h.close()
    return found


# ---- 6: the Python plugin --------------------------------------------------------------------------------------------------------------------------------
def b6_plugin(ctx, pr2, lib):
    """consistency_limits on the Python face of the plugin core (the C++ face and the hybrid path: tests/cpp/test_consistency_limits.cpp): the key, the windows,
    the seam, a pinned variable, the refusals, per-query rows, one call per pose"""
    from bio_ik_amd import BioIKKinematicsPlugin, KinematicsQueryOptions
    from bio_ik_amd.plugin import ConsistencyLimitsError, MoveItErrorCodes
    from conftest import random_configuration
    from test_plugin import goal_in_base_frame
    from bio_ik_amd.solver import sync_debug_switches
    arm = ("right_arm", "torso_lift_link", ["r_wrist_roll_link"])
    h = ctx.make_solver(template("arm", pr2))  # (the solver library behind the plugin re-reads its switches: the launcher's report is on for this test)
    sync_debug_switches(h.L)
    h.close()
    p = BioIKKinematicsPlugin(lib=lib)
    assert p.initialize(pr2, *arm, 0.0, params={"gpu_max_steps": 9, "random_seed": 3, "gpu_reproducible_calls": True, "gpu_islands": 1, "gpu_population": 16,
                                                "gpu_schedule": "latency"})
    assert p.params["gpu_consistency_limits"] is False
    rng = np.random.default_rng(29)
    gv = np.asarray(p._group_vars)
    G = len(gv)
    vmin, vmax = np.asarray(pr2.var_min)[gv], np.asarray(pr2.var_max)[gv]
    targets = np.tile(pr2.default_positions(), (N, 1))
    targets[:, gv] = vmin + (vmax - vmin) * (0.1 + 0.8 * rng.random((N, G)))
    poses = np.stack([goal_in_base_frame(pr2, x) for x in targets]).reshape(N, 1, 7)
    seeds = np.clip(targets[:, gv] + rng.uniform(-0.6, 0.6, (N, G)), vmin, vmax)
    approx = KinematicsQueryOptions(return_approximate_solution=True)
    c02 = [0.2] * G

    def single(k, limits, seed=None):
        sol, code = [], MoveItErrorCodes()
        ok = p.searchPositionIK(poses[k], list(seeds[k] if seed is None else seed), 0.0, sol, code, options=approx, consistency_limits=limits)
        return ok, np.array(sol), code.val

    # key off: the argument is ignored, whatever it holds
    free = [single(k, None)[1] for k in range(N)]
    for k in range(N):
        assert np.array_equal(single(k, c02)[1], free[k]) and np.array_equal(single(k, [-1.0] * G)[1], free[k])
    # key on, c = 0.2: within c of the seed, and another answer than the unlimited one for at least one query; an empty argument: unlimited
    p.params["gpu_consistency_limits"] = True
    differ = 0
    for k in range(N):
        ok, sol, code = single(k, c02)
        assert ok and code == MoveItErrorCodes.SUCCESS and (np.abs(sol - seeds[k]) <= 0.2).all() and (sol >= vmin).all() and (sol <= vmax).all()
        differ += int(not np.array_equal(sol, free[k]))
        assert np.array_equal(single(k, [])[1], free[k])
    assert differ >= 1
    # a continuous joint seeded at 3.1 stays in [2.9, pi]; c = 0 pins a variable
    cont = [i for i in range(G) if not pr2.var_bounded[gv[i]]]
    assert cont
    seed, c = seeds[0].copy(), list(c02)
    seed[cont[0]] = 3.1
    c[1] = 0.0
    ok, sol, code = single(0, c, seed)
    assert ok and 2.9 <= sol[cont[0]] <= np.pi and sol[1] == seed[1] and (np.abs(sol - seed) <= np.asarray(c)).all()
    seed[cont[0]] = -3.1
    ok, sol, code = single(0, c, seed)
    assert ok and -np.pi <= sol[cont[0]] <= -2.9
    # refused before any launch: searchPositionIK answers NO_IK_SOLUTION, the batched faces raise and name the variable
    ctx.report.read()
    bad = list(c02)
    bad[2] = -0.1
    outside = seeds[0].copy()
    outside[0] = vmax[0] + 0.5
    for limits, sd in ((bad, None), ([0.2] * (G - 1), None), ([float("nan")] * G, None), (c02, outside)):
        ok, sol, code = single(0, limits, sd)
        assert not ok and code == MoveItErrorCodes.NO_IK_SOLUTION
    name = pr2.variable_names[gv[2]]
    for call in (lambda: p.searchPositionIKBatch(poses, seeds, approx, consistency_limits=bad), lambda: p.searchPositionIKBatchAsync(poses, seeds, approx, consistency_limits=bad),
                 lambda: p.searchPositionIKEach(poses, seeds, approx, consistency_limits=bad)):
        try:
            call()
            raise AssertionError("a negative limit was accepted")
        except ConsistencyLimitsError as e:
            assert name in str(e), str(e)
    for limits in ([c02, c02], [[0.2] * (G + 1)]):
        try:
            p.searchPositionIKBatch(poses, seeds, approx, consistency_limits=limits)
            raise AssertionError("limits of the wrong shape were accepted")
        except ConsistencyLimitsError:
            pass
    assert not ctx.report.kernels(ctx.report.read()), "nothing launched"
    # the batched faces honour the argument whatever the key says: one shared row, a row per query, one call per pose
    p.params["gpu_consistency_limits"] = False
    shared = p.searchPositionIKBatch(poses, seeds, approx, consistency_limits=c02)[0]
    rows = np.array([[0.05 * (k + 1)] * G for k in range(N)])
    each = p.searchPositionIKBatch(poses, seeds, approx, consistency_limits=rows)[0]
    assert (np.abs(shared - seeds) <= 0.2).all() and (np.abs(each - seeds) <= rows).all()
    assert np.array_equal(each[3], shared[3]) and not np.array_equal(each[0], shared[0])
    assert ctx.report.kernels(ctx.report.read()) == ["k_solve_bounded"] * 2
    one_by_one = p.searchPositionIKEach(poses, seeds, approx, consistency_limits=rows)[0]
    assert (np.abs(one_by_one - seeds) <= rows).all() and np.array_equal(one_by_one[0], each[0])
    assert not np.array_equal(p.searchPositionIKBatch(poses, seeds, approx)[0], shared)
    p.close()
