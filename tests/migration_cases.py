"""Island migration (bioik_solve_params::island_migration, include/bioik_hip.h: ISLAND MIGRATION), shared by the host-simulator suite
(tests/test_hostsim_migration.py) and the GPU suite (tests/test_gpu_migration.py).

The oracle has no migration and its solver cannot be set to a state, so the RULE is checked where it can be isolated: bioik_eval_migrate runs the kernel a
solve runs at a boundary on rows the test makes up, against `restate` below -- the donor, the recipients and the words they change, written from the header's
text.  Whole solves are checked by identities (a call that cannot migrate is the call without the key), bit for bit against the host simulator of the same
kernel bodies, for determinism, for the result contract of tests/random_robot_cases.py, and for doing something at all.

`ctx` is the suite's context: make_solver(template) (the library under test), make_sim(template) (the host simulator), dev (streams and captures, as
sequence_cases), mp (monkeypatch), report (limit_cases.Report) or None."""
import contextlib
import ctypes as C

import numpy as np

from bio_ik_amd import JointVariableGoal, MinimalDisplacementGoal, PoseGoal, ProblemTemplate, abi
from bio_ik_amd.solver import BioIKError
from bio_ik_amd.workload import make_queries
from conftest import mimic_robot

NAMES = ("solutions", "fitness", "success", "steps")
DBL_MAX = np.finfo(np.float64).max


class Ctx:
    def __init__(self, make_solver, make_sim, dev, mp, report=None):
        self.make_solver, self.make_sim, self.dev, self.mp, self.report = make_solver, make_sim, dev, mp, report

    @contextlib.contextmanager
    def env(self, **kw):
        for k, v in kw.items():
            self.mp.setenv(k, v)
        try:
            yield
        finally:
            for k in kw:
                self.mp.delenv(k, raising=False)


# ---- the problems ------------------------------------------------------------------------------------------------------------------------------------------
_templates = {}


def template(name, pr2):
    """arm: the 7-DOF arm of the parity cases; mimic: ops that are no genes (conftest.mimic_robot); jv: a JointVariableGoal puts its variable in front of the
    chain's, so the genes do not follow the ops (the general kernel); sec: the arm with a secondary goal"""
    if name not in _templates:
        if name == "arm":
            t = ProblemTemplate(pr2, "right_arm", [PoseGoal("r_wrist_roll_link")])
        elif name == "mimic":
            t = ProblemTemplate(mimic_robot(), "arm", [PoseGoal("tool")])
        elif name == "jv":
            t = ProblemTemplate(pr2, "right_arm", [PoseGoal("r_wrist_roll_link"), JointVariableGoal("r_elbow_flex_joint", -1.0, weight=0.5)])
        elif name == "sec":
            t = ProblemTemplate(pr2, "right_arm", [PoseGoal("r_wrist_roll_link"), MinimalDisplacementGoal(weight=0.7)])
        else:
            raise KeyError(name)
        _templates[name] = t
    return _templates[name]


def queries(t, h, n, seed, **kw):
    return make_queries(t, h.active_variables, h.fk_genes, n, seed=seed, **kw)[:2]


def same(got, want, what):
    for name, x, y in zip(NAMES + ("count",), got, want):
        assert x.shape == y.shape and np.array_equal(x, y), "%s: %s differ" % (what, name)


def params(**kw):
    return abi.default_solve_params(**dict(dict(population=16, max_steps=9, random_seed=3), **kw))


# ---- 1: the rule against a restatement ---------------------------------------------------------------------------------------------------------------------
def restate(live, rows):
    """points 3 and 4 of the contract on rows [n][islands][9 M + 24]: per query the donor is the live island with the least solution fitness (word 20 of the
    bookkeeping), equal values: the lower island; every other live island with a STRICTLY greater figure takes the donor's solution into both elites of its
    rank-1 species, zero gradients, and the donor's figure into the two elites' fitness words (9, 10).  Nothing else changes."""
    n, islands, R = rows.shape
    M = (R - 24) // 9
    out = rows.copy()
    for q in range(n):
        alive = [i for i in range(islands) if live[q, i]]
        if len(alive) < 2:
            continue
        fit = rows[q, :, 9 * M + 20]
        donor = min(alive, key=lambda i: (fit[i], i))
        for i in alive:
            if i != donor and fit[i] > fit[donor]:
                sol = rows[q, donor, 8 * M:9 * M]
                out[q, i, 4 * M:5 * M] = sol
                out[q, i, 5 * M:6 * M] = 0.0
                out[q, i, 6 * M:7 * M] = sol
                out[q, i, 7 * M:8 * M] = 0.0
                out[q, i, 9 * M + 9] = out[q, i, 9 * M + 10] = fit[donor]
    return out


def made_up_rows(R, islands, rng):
    """six queries: [0] every island live, the least fitness held by TWO islands (the lower gives, the other stays: its figure is not greater); [1] one live
    island; [2] none; [3] island 0 dead with the least figure of all, the donor's figure repeated in a live island (it stays); [4] distinct figures, island 0 dead;
    [5] every figure equal (nobody receives)"""
    n, M = 6, (R - 24) // 9
    rows = rng.normal(size=(n, islands, R))
    rows[:, :, 9 * M + 20] = rng.random((n, islands)) + 1.0
    live = np.ones((n, islands), dtype=np.int32)
    a, b = sorted(rng.choice(islands, 2, replace=False))
    rows[0, a, 9 * M + 20] = rows[0, b, 9 * M + 20] = 0.5
    live[1] = 0
    live[1, islands - 1] = 1
    live[2] = 0
    live[3, 0] = 0
    rows[3, 0, 9 * M + 20] = 0.125
    rows[3, 1, 9 * M + 20] = rows[3, islands - 1, 9 * M + 20] = 0.75
    live[4, 0] = 0
    live[4, islands // 2] = 0
    rows[5, :, 9 * M + 20] = 2.0
    live[0, :] = 7  # (any non-zero value is "live")
    return live, rows


def m1_rule(ctx, pr2, name, islands):
    t = template(name, pr2)
    h = ctx.make_solver(t)
    R = h.carry_doubles()
    M = (R - 24) // 9
    assert R == 9 * M + 24 and M >= h.D
    if name == "mimic":
        assert M > h.D, "precondition: more ops than genes"
    rng = np.random.default_rng(100 + islands)
    live, rows = made_up_rows(R, islands, rng)
    want = restate(live, rows)
    got = h.migrate(live, rows)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "bioik_eval_migrate differs from the restated rule at (query, island, word) %s" % (
        np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:8].tolist())
    # (the cases are what the docstring says they are)
    changed = (want.view(np.uint64) != rows.view(np.uint64)).any(axis=2)
    assert changed[0].sum() == islands - 2 and not changed[1].any() and not changed[2].any() and not changed[5].any()
    assert not changed[3, 0] and not changed[3, 1] and not changed[3, islands - 1] and changed[3].sum() == islands - 3
    assert changed[4].sum() == islands - 3
    h.close()


# ---- 2: identities of whole solves -------------------------------------------------------------------------------------------------------------------------
def m2_identities(ctx, pr2):
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp = queries(t, h, 3, 5)
    off = h.solve_batch(params(islands=3), seeds, gp)
    for e in (9, 12):
        same(h.solve_batch(params(islands=3, island_migration=e), seeds, gp), off, "E = %d >= max_steps" % e)
    one = h.solve_batch(params(islands=1), seeds, gp)
    same(h.solve_batch(params(islands=1, island_migration=2), seeds, gp), one, "one island")
    # island_sync: a query the call without migration finishes within E steps never reaches a boundary
    s2, g2 = queries(t, h, 8, 6, kind="tracking", noise=0.002)
    for e in (2, 3):
        off = h.solve_batch(params(islands=3, island_sync=1), s2, g2)
        on = h.solve_batch(params(islands=3, island_sync=1, island_migration=e), s2, g2)
        early = (off[2] != 0) & (off[3] <= e)
        assert early.any() and not early.all(), "precondition: queries that finish within %d steps, and others (%s)" % (e, off[3])
        same([x[early] for x in on], [x[early] for x in off], "island_sync, finished within E = %d" % e)
    if ctx.report is not None:  # ... and the very plan of E = 0: the same launches
        for islands, e in ((1, 2), (3, 9)):
            ctx.report.read()
            h.solve_batch(params(islands=islands), seeds, gp)
            want = ctx.report.kernels(ctx.report.read())
            h.solve_batch(params(islands=islands, island_migration=e), seeds, gp)
            got = ctx.report.kernels(ctx.report.read())
            assert want and got == want and "k_migrate_mark" not in got, (want, got)
    h.close()


# ---- 3: the library under test against the host simulator --------------------------------------------------------------------------------------------------
# (problem, queries, islands, E, island_sync, max_steps): every value of every dimension of the issue's list, and the cap crossed (40 steps, E = 2: 19 steps below
# max_steps are multiples of 2, 8 boundaries are taken)
SOLVES = {
    "arm_n3_i2_e2": ("arm", 3, 2, 2, 0, 9),
    "arm_n1_i3_e3_sync": ("arm", 1, 3, 3, 1, 9),
    "arm_n1_i64_e2_sync": ("arm", 1, 64, 2, 1, 9),
    "arm_n1_i65_e3": ("arm", 1, 65, 3, 0, 9),
    "mimic_n3_i3_e2": ("mimic", 3, 3, 2, 0, 9),
    "mimic_n1_i2_e3_sync": ("mimic", 1, 2, 3, 1, 9),
    "jv_n3_i3_e3": ("jv", 3, 3, 3, 0, 9),
    "jv_n1_i65_e2_sync": ("jv", 1, 65, 2, 1, 9),
    "sec_n3_i3_e2": ("sec", 3, 3, 2, 0, 9),
    "arm_n1_i3_e2_cap": ("arm", 1, 3, 2, 0, 40),
    "arm_linear_n3_i3_e2": ("arm", 3, 3, 2, 0, 9, dict(fk_mode=abi.FK_LINEAR)),  # linearised phenotypes: the elites' fitness words are not written (every generation re-evaluates them)
}
_sim_results = {}


def solve_case(h, pr2, name, **kw):
    prob, n, islands, e, sync, steps = SOLVES[name][:6]
    kw = dict(SOLVES[name][6] if len(SOLVES[name]) > 6 else {}, **kw)
    t = template(prob, pr2)
    seeds, gp = queries(t, h, n, 20 + n)
    return h.solve_batch(params(islands=islands, island_migration=e, island_sync=sync, max_steps=steps, **kw), seeds, gp)


def simulated(ctx, pr2, name):
    """the host simulator's result of a case: computed once, shared, never changed"""
    if name not in _sim_results:
        s = ctx.make_sim(template(SOLVES[name][0], pr2))
        _sim_results[name] = tuple(np.array(x, copy=True) for x in solve_case(s, pr2, name))
        for x in _sim_results[name]:
            x.setflags(write=False)
        s.close()
    return _sim_results[name]


def m3_against_simulator(ctx, pr2, name):
    h = ctx.make_solver(template(SOLVES[name][0], pr2))
    if ctx.report is not None:
        ctx.report.read()
    got = solve_case(h, pr2, name)
    if ctx.report is not None:
        prob, n, islands, e, sync, steps = SOLVES[name][:6]
        k = ctx.report.kernels(ctx.report.read())
        boundaries = min(abi.MAX_MIGRATIONS, (steps - 1) // e)
        assert k.count("k_migrate_mark") == boundaries and len([x for x in k if x.startswith("k_solve")]) == boundaries + 1, k
        assert k[-1] in ("k_select", "k_select_wave"), k  # (never the fused reduction)
    if ctx.make_sim is ctx.make_solver and name not in _sim_results:  # (the simulator's own suite: this IS the shared result; later tests hold theirs against it)
        _sim_results[name] = tuple(np.array(x, copy=True) for x in got)
    same(got, simulated(ctx, pr2, name), name + " against the host simulator")
    h.close()


def m3_ranked(ctx, pr2):
    t = template("arm", pr2)
    h, s = ctx.make_solver(t), ctx.make_sim(t)
    seeds, gp = queries(t, h, 3, 31)
    kw = dict(islands=3, island_migration=2)
    got = h.solve_batch_ranked(params(**kw), seeds, gp, 2, -1.0)
    same(got, s.solve_batch_ranked(params(**kw), seeds, gp, 2, -1.0), "ranked, against the host simulator")
    plain = h.solve_batch(params(island_sync=0, **kw), seeds, gp)
    for nm, x, y in zip(NAMES, got[:4], plain):
        assert np.array_equal(x[:, 0], y), "row 0 of %s is not the plain call's" % nm
    h.close(), s.close()


# ---- 4: determinism ----------------------------------------------------------------------------------------------------------------------------------------
MAPPINGS = ({"BIOIK_SOLVE_THREADS": "64"}, {"BIOIK_SOLVE_THREADS": "128", "BIOIK_SOLVE_GENERAL": "1"})


def m4_determinism(ctx, pr2, name="arm_n1_i64_e2_sync"):
    h = ctx.make_solver(template(SOLVES[name][0], pr2))
    first = solve_case(h, pr2, name)
    same(solve_case(h, pr2, name), first, "the same call twice")
    for env in MAPPINGS:
        with ctx.env(**env):
            same(solve_case(h, pr2, name), first, "under %s" % env)
    h.close()


# ---- 5: it does something, and what it returns keeps the result contract -------------------------------------------------------------------------------------
def m5_does_something(ctx, pr2):
    """Queries: the 7-DOF arm, make_queries(seed=40), 6 queries, population 16, 3 islands, 9 steps, random_seed 3.  Chosen on the host simulator: with migration
    off all 6 of 6 returned islands are still running after step 2 (steps 6 7 9 9 9 9: 100 %; two of them succeed), and with E = 2 the results of 6 of the 6 queries differ (a third one succeeds)."""
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp = queries(t, h, 6, 40)
    e = 2
    off = h.solve_batch(params(islands=3), seeds, gp)
    assert (off[3] > e).sum() * 2 >= len(off[3]), "precondition: at least half of the queries still run after step %d without migration (steps %s)" % (e, off[3])
    on = h.solve_batch(params(islands=3, island_migration=e), seeds, gp)
    differs = [q for q in range(6) if any(not np.array_equal(a[q], b[q]) for a, b in zip(on, off))]
    assert differs, "island_migration = %d changed no query's result" % e
    many = 5 if ctx.make_sim is ctx.make_solver else 65  # (65 islands of four queries take the simulator most of a minute: the device's share)
    for tn, n_q, kw in (("arm", 6, dict(islands=3)), ("sec", 4, dict(islands=3, island_sync=1)), ("jv", 4, dict(islands=many, island_sync=1))):
        tt = template(tn, pr2)
        hh = h if tn == "arm" else ctx.make_solver(tt)
        s, g = (seeds, gp) if tn == "arm" else queries(tt, hh, n_q, 41)
        result_contract(hh, tt, params(island_migration=e, **kw), s, g)
        if hh is not h:
            hh.close()
    h.close()
    return len(differs), off[3]


def result_contract(h, t, p, seeds, gp):
    """the part of tests/random_robot_cases.result_contract that needs no second implementation: the returned fitness is bioik_eval_fitness of the returned solution
    (plus the secondary term of a success), the success flag bioik_eval_check of it, steps within the budget, inactive variables the seed's"""
    sol, fit, suc, steps = h.solve_batch(p, seeds, gp)
    act = np.asarray(h.active_variables)
    inactive = np.setdiff1d(np.arange(sol.shape[1]), act)
    assert np.array_equal(sol[:, inactive], seeds[:, inactive])
    assert ((steps >= 1) & (steps <= p.max_steps)).all(), steps
    has_sec = any(g.isSecondary() for g in t.goals)
    for q in range(len(fit)):
        if fit[q] == DBL_MAX:
            assert np.array_equal(sol[q], seeds[q]) and not suc[q]
            continue
        genes = sol[q][act][None, :]
        pa, sa = h.fitness(abi.FK_EXACT, seeds[q], gp[q], genes)
        want = pa[0] + sa[0] if (suc[q] and has_sec) else pa[0]
        assert fit[q] == want, "query %d (success %d): fitness %.17g, eval_fitness of the solution %.17g + %.17g" % (q, suc[q], fit[q], pa[0], sa[0])
        assert int(h.check(p, seeds[q], gp[q], genes)[0]) == int(suc[q]), "query %d: success %d, eval_check of the solution says otherwise" % (q, suc[q])


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------------------------
def m6_refusals(ctx, pr2):
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp = queries(t, h, 2, 50)

    def code(call):
        try:
            call()
            return abi.OK
        except BioIKError as e:
            assert str(e)
            return e.code

    assert code(lambda: h.solve_batch(params(islands=3, island_migration=-1), seeds, gp)) == abi.ERR_INVALID_ARGUMENT
    assert code(lambda: h.solve_batch(params(islands=1, island_migration=-2), seeds, gp)) == abi.ERR_INVALID_ARGUMENT
    for mode in ("gd", "gd_r", "gd_c", "jac"):
        assert code(lambda: h.solve_batch(params(islands=3, island_migration=2, mode=mode), seeds, gp)) == abi.ERR_UNSUPPORTED, mode
        assert code(lambda: h.solve_batch(params(islands=3, island_migration=0, mode=mode, max_steps=2), seeds, gp)) == abi.OK, mode
    assert code(lambda: h.solve_batch_ranked(params(islands=3, island_migration=-1), seeds, gp, 2)) == abi.ERR_INVALID_ARGUMENT
    # bad arguments of the function-level entry
    R = h.carry_doubles()
    rows, live = np.zeros((1, 2, R)), np.ones((1, 2), dtype=np.int32)
    assert h.L.bioik_eval_migrate(h.problem, 0, 1, live.ctypes.data_as(C.POINTER(C.c_int32)), rows.ctypes.data_as(C.POINTER(C.c_double))) == abi.ERR_INVALID_ARGUMENT
    assert h.L.bioik_eval_migrate(h.problem, 2, 1, None, rows.ctypes.data_as(C.POINTER(C.c_double))) == abi.ERR_INVALID_ARGUMENT
    assert h.L.bioik_eval_migrate(h.problem, 2, 0, None, None) == abi.OK
    h.close()


def m6_capture(ctx, pr2):
    """a call that would migrate is refused on a capturing stream; the call that cannot migrate (one island) is the call E = 0 is, and is captured like it"""
    t = template("arm", pr2)
    h = ctx.make_solver(t)
    seeds, gp = queries(t, h, 2, 51)
    b = ctx.dev.buf
    ins = (b(np.ascontiguousarray(seeds)), b(np.ascontiguousarray(gp)))
    outs = (b(np.zeros((2, h.V))), b(np.zeros(2)), b(np.zeros(2, dtype=np.int32)), b(np.zeros(2, dtype=np.int32)))
    ptrs = [x.ptr for x in ins + outs]
    s = ctx.dev.stream(3)
    codes = []

    def enqueue():
        with ctx.dev.on(s):
            try:
                h.solve_batch_device(params(islands=3, island_migration=2), 2, *ptrs, ctx.dev.handle(s))
                codes.append(abi.OK)
            except BioIKError as e:
                codes.append(e.code)

    enqueue()  # eager: accepted
    ctx.dev.sync()
    eager = tuple(o.get() for o in outs)
    same(eager, h.solve_batch(params(islands=3, island_migration=2), seeds, gp), "the device-pointer entry")
    g = ctx.dev.capture(s, enqueue)
    ctx.dev.destroy(g)
    assert codes == [abi.OK, abi.ERR_UNSUPPORTED], codes
    h.close()


# ---- 6: the Python plugin's key ------------------------------------------------------------------------------------------------------------------------------
def m6_plugin_key(ctx, pr2, lib):
    """gpu_island_migration of bio_ik_amd.plugin reaches the device: the launcher reports the migration launches, and only with the key set"""
    from bio_ik_amd import BioIKKinematicsPlugin, KinematicsQueryOptions
    from conftest import random_configuration
    from test_plugin import goal_in_base_frame
    arm = ("right_arm", "torso_lift_link", ["r_wrist_roll_link"])
    p = BioIKKinematicsPlugin(lib=lib)
    assert p.initialize(pr2, *arm, 0.0, params={"gpu_max_steps": 5, "random_seed": 5, "gpu_reproducible_calls": True, "gpu_islands": 3, "gpu_population": 16,
                                                "gpu_island_sync": False})
    assert p.params["gpu_island_migration"] == 0
    rng = np.random.default_rng(23)
    gv = p._group_vars
    n = 2
    targets = np.tile(pr2.default_positions(), (n, 1))
    targets[:, gv] = random_configuration(pr2, rng, n)[:, gv]
    poses = np.stack([goal_in_base_frame(pr2, x) for x in targets]).reshape(n, 1, 7)
    seeds = random_configuration(pr2, rng, n)[:, gv]
    approx = KinematicsQueryOptions(return_approximate_solution=True)
    ctx.report.read()
    off = p.searchPositionIKBatch(poses, seeds, options=approx)[0]
    k_off = ctx.report.kernels(ctx.report.read())
    p.params["gpu_island_migration"] = 2
    on = p.searchPositionIKBatch(poses, seeds, options=approx)[0]
    k_on = ctx.report.kernels(ctx.report.read())
    p.close()
    assert "k_migrate_mark" not in k_off and k_on.count("k_migrate_mark") == 2, (k_off, k_on)  # (5 steps, E = 2: boundaries after steps 2 and 4)
    assert off.shape == on.shape
