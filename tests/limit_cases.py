"""Limit cases shared by the host-simulator suite (tests/test_hostsim_limits.py) and the GPU suite (tests/test_gpu_limits.py): every entry point at
the problem-size limits include/bioik_hip.h declares (63 active variables, 64 ops, 64 tips, 24 + 24 goals, 4 BalanceGoals), the launcher's mapping
thresholds seen from both sides, and the LDS envelope of every entry point (just under 64 KiB, just over, beyond a CU's 160 KiB).

`make_solver(template)` builds a bio_ik_amd.solver.HipSolver on the library under test.  The oracle runs in device-arithmetic mode (trig mode 1, set by
the calling suite) and results are compared bit for bit, except where a docstring says otherwise.  A problem the library cannot hold must be refused
with BIOIK_ERR_UNSUPPORTED -- never BIOIK_ERR_HIP."""
import re

import numpy as np
import pytest

import np_fk
import parity_cases as pc
from bio_ik_amd import (AvoidJointLimitsGoal, BalanceGoal, CenterJointsGoal, DirectionGoal, JointVariableGoal, LookAtGoal, MinimalDisplacementGoal,
                        OrientationGoal, PoseGoal, PositionGoal, ProblemTemplate, RobotModel, abi, snake)
from bio_ik_amd.solver import BioIKError
from bio_ik_amd.workload import make_queries
from conftest import random_configuration
from oracle import orc

KIB = 1024
LDS_CU = 160 * KIB  # LDS of an MI355X CU (the host simulator stands for one)


# ---- the layout arithmetic (bio_ik_amd/csrc: make_layout at lambda = 0, make_point_layout, eval_reproduce_body) ---------------------------------
def eval_lds(n_ops, V, P, T, n_slots, nth=64):
    """bytes of dynamic LDS of k_eval_fk / _fitness / _approximator / _check / k_stream_fitness at `nth` lanes: seed, goal parameters, two elite
    buffers, the solution, clip table, a genotype column per lane, parked frames per lane; then the group: line-search vectors, the four frame sets,
    tip frames, the approximator's 7 T m table, reduction and broadcast slots"""
    m = max(n_ops, 1)
    o = V + max(P, 1) + 16 * m + m + 8 + 24 + 2 * m + m * nth + n_slots * 7 * nth
    g = 9 * m
    g += g & 1
    g += 32 * max(T, 1) + 7 * T + 7 * T * m + m + 4 * (nth // 64) + 4 + 4
    return (o + g) * 8


def reproduce_lds(n_ops, nth=64):
    """bytes of k_eval_reproduce: the two parents (genes | momentum) and a genotype and a gradient column per lane"""
    m = max(n_ops, 1)
    return (4 * m + 2 * m * nth) * 8


def point_lds(n_ops, V, P, T, n_slots, D, nth=64):
    """bytes of k_solve_point (gd_c, jac): the configuration, gradient, a column per lane, the frame chain, the 6T x D Jacobian twice, the SVD's V"""
    m, d, t6 = max(n_ops, 1), max(D, 1), 6 * max(T, 1)
    q = min(d, t6)
    return (V + max(P, 1) + 8 + 3 * m + d + 8 + m * nth + n_slots * 7 * nth + 7 * m + 7 * max(T, 1) + 2 * t6 * d + q * q + q + t6 + d) * 8


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def refused(call):
    """`call` must fail with BIOIK_ERR_UNSUPPORTED"""
    with pytest.raises(BioIKError) as e:
        call()
    assert e.value.code == abi.ERR_UNSUPPORTED, str(e.value)


def runs_or_refused(call):
    """the result of `call`, or None when it was refused with BIOIK_ERR_UNSUPPORTED (any other error fails the test)"""
    try:
        return call()
    except BioIKError as e:
        assert e.code == abi.ERR_UNSUPPORTED, str(e)
        return None


class Report:
    """BIOIK_SOLVE_REPORT=1 and the library's stderr (pytest's capfd): what the launcher printed since the last read"""

    def __init__(self, monkeypatch, capfd):
        monkeypatch.setenv("BIOIK_SOLVE_REPORT", "1")
        self.capfd = capfd
        self.read()

    def read(self):
        return self.capfd.readouterr().err

    def shape(self, text):
        """(ops, genes, tips, slots) of the last mapping report in `text`"""
        found = re.findall(r"\[bioik\] solve: ops (\d+) genes (\d+) tips (\d+) slots (\d+)", text)
        assert found, text[-2000:]
        return tuple(int(x) for x in found[-1])

    def kernels(self, text):
        return re.findall(r"\[bioik\] launch: (k_\w+)", text)


def shape_of(h, t, report):
    """(ops, genes, tips, slots) of a problem, from the mapping report of a one-query, one-step solve"""
    seeds, params, _ = make_queries(t, h.active_variables, h.fk_genes, 1, seed=3)
    report.read()
    h.solve_batch(abi.default_solve_params(population=16, max_steps=1, random_seed=1), seeds, params)
    return report.shape(report.read())


def chain(n, mimic_at=(), link_length=0.1):
    """snake(n) with a mimic joint behind segment k for every k of `mimic_at` (it follows joint j1; no gene of its own): n + len(mimic_at) ops, n genes"""
    m = RobotModel("chain%d_%d" % (n, len(mimic_at)))
    m.add_link("base")
    prev = "base"
    for k in range(n):
        m.add_link("seg%d" % k, prev, "j%d" % k, "revolute", xyz=(link_length if k else 0.0, 0, 0), axis=(0, 1, 0) if k % 2 == 0 else (0, 0, 1),
                   lower=-1.5, upper=1.5, velocity=1.0)
        prev = "seg%d" % k
        if k in mimic_at:
            m.add_link("mim%d" % k, prev, "m%d" % k, "revolute", xyz=(0.05, 0, 0), axis=(0, 0, 1), lower=-1.5, upper=1.5, velocity=1.0, mimic=("j1", 0.5, 0.1))
            prev = "mim%d" % k
    m.add_link("tip", prev, "tip_joint", "fixed", xyz=(link_length, 0, 0))
    m.add_group("snake", chain=("base", "tip"))
    return m


def centipede(n_seg=16, legs=48, extra=0):
    """Test fixture: a spine of `n_seg` revolute joints (alternating y / z axes, axis-aligned origins) whose links carry a mass, `legs` massive links on
    fixed joints spread over the segments round-robin, and `extra` massive links on the base.  A BalanceGoal makes every massive link a tip: n_seg + legs
    + extra tips, n_seg ops, no parked frames."""
    m = RobotModel("centipede%d_%d_%d" % (n_seg, legs, extra))
    m.add_link("base")
    prev = "base"
    for k in range(n_seg):
        m.add_link("seg%d" % k, prev, "j%d" % k, "revolute", xyz=(0.08 if k else 0.0, 0, 0.0), axis=(0, 1, 0) if k % 2 == 0 else (0, 0, 1), lower=-1.2,
                   upper=1.2, velocity=1.0, mass=1.0 + 0.1 * (k % 3), com=(0.04, 0.0, 0.0))
        prev = "seg%d" % k
    for i in range(legs):
        k, side = i % n_seg, i // n_seg
        m.add_link("leg%d" % i, "seg%d" % k, "leg%d_joint" % i, "fixed", xyz=(0.02, (0.05 + 0.01 * side) * (1 if side % 2 == 0 else -1), -0.01 * side),
                   mass=0.2 + 0.05 * side, com=(0.0, 0.0, -0.02))
    for i in range(extra):
        m.add_link("ballast%d" % i, "base", "ballast%d_joint" % i, "fixed", xyz=(-0.05, 0.01 * i, 0.0), mass=2.0)
    m.add_group("body", chain=("base", "seg%d" % (n_seg - 1)))
    return m


def position_chain(n, n_goals):
    """snake-like chain of n joints with PositionGoals on the last `n_goals` segment links (listed in walk order): n ops, n_goals tips, no parked frames"""
    m = snake(n)
    goals = [PositionGoal("seg%d" % k, (0.1 * (k % 5), 0.05, 0.02 * (k % 3)), weight=0.5 + 0.01 * k) for k in range(n - n_goals, n)]
    return m, ProblemTemplate(m, "snake", goals)


# ---- 1. D = 63 -----------------------------------------------------------------------------------------------------------------------------------
def d63(make_solver, report):
    """63 active variables on one chain: the function level (reproduce needs 66,528 B of LDS here: more than 64 KiB, allowed explicitly), whole solves at
    populations 16, 70 and 128 (exact FK) and 70 (linear FK), and the point solvers gd_c / jac -- which run when their layout fits 64 KiB (it does here:
    about 44 KiB) and are refused otherwise."""
    m = snake(63)
    t = ProblemTemplate(m, "snake", [PoseGoal("tip"), AvoidJointLimitsGoal(weight=0.3)])
    h, o = make_solver(t), orc.Oracle(t)
    assert h.D == o.D == 63
    ops, genes, tips, slots = shape_of(h, t, report)
    assert (ops, genes, tips, slots) == (63, 63, 1, 0)
    assert reproduce_lds(ops) == 66528
    pc.function_level(h, o, m, np.random.default_rng(63), n=70, exact_bits=True)
    for pop in (16, 70, 128):
        pc.trajectory(h, o, t, n=2, pop=pop, steps_list=(1, 2))
    pc.trajectory(h, o, t, n=2, pop=70, steps_list=(2,), fk_mode=abi.FK_LINEAR)
    fits = point_lds(ops, h.V, h.P, tips, slots, genes) <= 64 * KIB
    assert fits
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, 2, seed=41, kind="tracking")
    for mode, st in (("gd_c", 3), ("jac", 2)):
        p = abi.default_solve_params(mode=mode, max_steps=st, random_seed=7)
        a = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=2)
        b = h.solve_batch(p, seeds, params)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), mode
    return h, t


# ---- 2. 64 ops with 63 genes ---------------------------------------------------------------------------------------------------------------------
def ops64(make_solver, report):
    """A 63-gene chain with a mimic joint in its middle: 64 ops, the last of them a gene (bit 63 of the active-op mask), the mimic follower's bit in the
    middle of the follower mask.  The function level and whole solves bit for bit; a second mimic joint (65 ops) is refused."""
    m = chain(63, mimic_at=(31,))
    t = ProblemTemplate(m, "snake", [PoseGoal("tip")])
    h, o = make_solver(t), orc.Oracle(t)
    assert h.D == o.D == 63
    assert shape_of(h, t, report)[:2] == (64, 63)
    pc.function_level(h, o, m, np.random.default_rng(64), n=40, exact_bits=True)
    pc.trajectory(h, o, t, n=2, pop=16, steps_list=(1, 3))
    pc.trajectory(h, o, t, n=1, pop=70, steps_list=(2,))
    pc.trajectory(h, o, t, n=1, pop=24, steps_list=(2,), fk_mode=abi.FK_LINEAR)
    refused(lambda: make_solver(ProblemTemplate(chain(63, mimic_at=(20, 40)), "snake", [PoseGoal("tip")])))
    refused(lambda: make_solver(ProblemTemplate(snake(65), "snake", [PoseGoal("tip")])))


# ---- 3. D = 32 and D = 33 ------------------------------------------------------------------------------------------------------------------------
def d32_33(make_solver, report, monkeypatch):
    """The `D < 32` rules seen from above: the throughput schedule's mapping (both species on the halves of one wavefront, the memetic phase on lane D
    of a group) is not taken -- both schedules give the same bits as the oracle --, and BIOIK_SOLVE_SPECIES_PARALLEL=1 at 64 lanes does not split the
    species over half-waves.  D = 31 on the same chain is the control: there it does."""
    for n in (31, 32, 33):
        m = snake(n)
        t = ProblemTemplate(m, "snake", [PoseGoal("tip")])
        h, o = make_solver(t), orc.Oracle(t)
        assert h.D == n
        res = []
        for sched in (abi.SCHEDULE_LATENCY, abi.SCHEDULE_THROUGHPUT):
            pc.trajectory(h, o, t, n=2, pop=128, steps_list=(2,), schedule=sched)
            seeds, params, _ = make_queries(t, h.active_variables, h.fk_genes, 2, seed=7)
            res.append(h.solve_batch(abi.default_solve_params(population=128, max_steps=2, random_seed=11, schedule=sched), seeds, params))
        assert all(np.array_equal(x, y) for x, y in zip(*res))
        monkeypatch.setenv("BIOIK_SOLVE_THREADS", "64")
        monkeypatch.setenv("BIOIK_SOLVE_SPECIES_PARALLEL", "1")
        report.read()
        pc.trajectory(h, o, t, n=1, pop=24, steps_list=(2,))
        text = report.read()
        assert ("species_parallel 1" in text) == (n < 32), text[-600:]
        monkeypatch.delenv("BIOIK_SOLVE_THREADS")
        monkeypatch.delenv("BIOIK_SOLVE_SPECIES_PARALLEL")


# ---- 4. T = 64 -----------------------------------------------------------------------------------------------------------------------------------
def t64(make_solver, report, steps=(1, 2)):
    """64 tips: 12 massive spine links, 52 massive legs, a BalanceGoal and a PoseGoal on the last segment.  FK of all 64 tips bit for bit against the
    oracle, and the oracle against tests/np_fk.py (long double, rotation matrices) to 1e-12; fitness to test_balance_goal's tolerances (the device sums
    the centre of mass in walk order, the reference in link order); short whole solves.  The function level needs 72,464 B of LDS here (more than
    64 KiB: allowed explicitly).  A 65th massive link is refused."""
    m = centipede(12, 52)
    t = ProblemTemplate(m, "body", [PoseGoal("seg11", (0.6, 0.3, 0.2), weight=0.5), BalanceGoal((0.3, 0.0, 0.0), weight=0.8)])
    h, o = make_solver(t), orc.Oracle(t)
    assert h.T == o.T == 64 and h.D == 12
    pc.assert_same_structure(h, o)
    rng = np.random.default_rng(65)
    full = random_configuration(m, rng, 12)
    genes = full[:, o.active_variables]
    a = o.fk_genes(full[0], genes)
    b = h.fk_genes(full[0], genes)
    assert np.array_equal(a, b)
    assert eval_lds(12, h.V, h.P, 64, 0) == 72464
    # the oracle's quaternion FK against rotation matrices in long double
    tips = o.fk(full)
    for k in range(full.shape[0]):
        R, p = np_fk.fk_all(m, full[k])
        for i, link in enumerate(o.tip_links):
            assert np.abs(tips[k, i, :3] - np.asarray(p[link], dtype=np.float64)).max() < 1e-12
            assert np.abs(np_fk.quat_to_rot64(tips[k, i, 3:]) - np.asarray(R[link], dtype=np.float64)).max() < 1e-12
    pc.function_level(h, o, m, rng, n=40, frame_tol=1e-12, fit_rtol=1e-10)
    for pop, kw in ((16, {}), (24, {"fk_mode": abi.FK_LINEAR}), (70, {})):
        balance_solves(h, o, t, pop, steps, **kw)
    refused(lambda: make_solver(ProblemTemplate(centipede(12, 52, extra=1), "body", [PoseGoal("seg11"), BalanceGoal()])))
    return h, t


def balance_solves(h, o, t, pop, steps, n=2, **kw):
    """Whole solves with a BalanceGoal: the device sums the centre of mass in walk order, the oracle in link order, so the two searches may part after
    the first tie that rounding decides -- what is compared is the device's answer under the oracle: every returned fitness is the oracle's exact
    fitness of the returned configuration (to rounding), and a solve never returns something worse than its seed."""
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, n, seed=17)
    for st in steps:
        sol, fit, suc, stp = h.solve_batch(abi.default_solve_params(population=pop, max_steps=st, random_seed=11, **kw), seeds, params)
        assert (stp >= 1).all() and (stp <= st).all()
        for k in range(n):
            want = o.fitness(abi.FK_EXACT, sol[k], params[k], sol[k][o.active_variables][None, :])[0][0]
            start = o.fitness(abi.FK_EXACT, seeds[k], params[k], seeds[k][o.active_variables][None, :])[0][0]
            assert abs(fit[k] - want) <= 1e-10 * abs(want) + 1e-15, (pop, st, k, fit[k], want)
            assert want <= start * (1 + 1e-10) + 1e-15, (pop, st, k)


# ---- 5. 24 + 24 goals, 4 BalanceGoals --------------------------------------------------------------------------------------------------------
def goals_24_24(make_solver):
    """24 primary goals of mixed kinds on a 31-joint chain (listed in walk order) and 24 secondary goals: the function level and whole solves bit for
    bit.  The 25th goal of either class is refused; so is a 5th BalanceGoal, while four of them run (to test_balance_goal's tolerances)."""
    m = snake(31)
    kinds = (lambda k: PositionGoal("seg%d" % k, (0.1, 0.02 * k, 0.0), weight=0.3),
             lambda k: OrientationGoal("seg%d" % k, (0.0, 0.1, 0.0, 0.99), weight=0.2),
             lambda k: PoseGoal("seg%d" % k, (0.2, 0.0, 0.01 * k), weight=0.4),
             lambda k: LookAtGoal("seg%d" % k, (1, 0, 0), (1.0, 0.5, 0.2), weight=0.1),
             lambda k: DirectionGoal("seg%d" % k, (0, 0, 1), (0, 1, 0), weight=0.15))
    prim = [kinds[i % len(kinds)](7 + i) for i in range(24)]

    def secondary(i):
        g = (MinimalDisplacementGoal, AvoidJointLimitsGoal, CenterJointsGoal)[i % 3](weight=0.1 + 0.01 * i) if i % 4 else \
            JointVariableGoal("j%d" % i, 0.1, weight=0.2, secondary=True)
        g.secondary_ = True
        return g
    sec = [secondary(i) for i in range(24)]
    t = ProblemTemplate(m, "snake", prim + sec)
    h, o = make_solver(t), orc.Oracle(t)
    pc.function_level(h, o, m, np.random.default_rng(24), n=40, exact_bits=True)
    pc.trajectory(h, o, t, n=2, pop=16, steps_list=(2,))
    pc.trajectory(h, o, t, n=1, pop=70, steps_list=(1,))
    refused(lambda: make_solver(ProblemTemplate(m, "snake", prim + [PositionGoal("tip")] + sec)))
    refused(lambda: make_solver(ProblemTemplate(m, "snake", prim + sec + [secondary(1)])))
    # four BalanceGoals (and a pose), then five
    b = centipede(6, 6)
    bal = [BalanceGoal((0.1 * i, 0.0, 0.0), weight=0.2 + 0.1 * i) for i in range(4)]
    t4 = ProblemTemplate(b, "body", [PoseGoal("seg5", (0.3, 0.1, 0.1))] + bal)
    h4, o4 = make_solver(t4), orc.Oracle(t4)
    pc.function_level(h4, o4, b, np.random.default_rng(4), n=40, frame_tol=1e-12, fit_rtol=1e-10)
    balance_solves(h4, o4, t4, 16, (2,))
    refused(lambda: make_solver(ProblemTemplate(b, "body", [PoseGoal("seg5")] + bal + [BalanceGoal()])))


# ---- 6. population thresholds ----------------------------------------------------------------------------------------------------------------
POPULATIONS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 4096)
# the kernel the launcher picks for a call of a few queries, where it is one of the kernels compiled for one mapping (BIOIK_SOLVE_REPORT): a rule change
# that moves one of these cases off its kernel fails here
# (k_solve_lean_cl4h: the helped build for launches that leave most of the chip idle, serial chains from 128 children on)
THRESHOLD_KERNELS = {("c2", p): "k_solve_lean_cl4h" for p in (128, 129, 255, 256, 257, 1024)}
THRESHOLD_KERNELS.update({("c4", p): "k_solve_lean_cl4h" for p in (128, 129, 255, 256, 257)})
THRESHOLD_KERNELS.update({("c4", p): "k_solve_lean_cl" for p in (33, 63, 64, 65, 127)})


def population_threshold(h, o, t, cfg, pop, report):
    """one population on C2 / C3 / C4: the oracle's trajectories bit for bit, or a refusal with BIOIK_ERR_UNSUPPORTED; the kernel it ran where
    THRESHOLD_KERNELS names one.  (Population 1 only without a secondary goal: the pre-selection keeps at least two children.)"""
    n, steps = (2, (1, 2)) if pop <= 257 else (1, (1,))
    report.read()
    got = runs_or_refused(lambda: pc.trajectory(h, o, t, n=n, pop=pop, steps_list=steps) or True)
    text = report.read()
    assert got, "population %d refused on %s" % (pop, cfg)
    ran = set(report.kernels(text))
    assert ran, text[-600:]
    want = THRESHOLD_KERNELS.get((cfg, pop))
    if want:
        assert ran == {want}, (cfg, pop, ran)
    return sorted(ran)


def small_linear_kernel(h, o, t, report):
    """populations up to 32 per species with linearised phenotypes run k_solve_lean_lin, 33 and more do not"""
    for pop, lin in ((16, True), (31, True), (32, True), (33, False)):
        report.read()
        pc.trajectory(h, o, t, n=2, pop=pop, steps_list=(2,), fk_mode=abi.FK_LINEAR)
        ran = set(report.kernels(report.read()))
        assert (ran == {"k_solve_lean_lin"}) == lin, (pop, ran)


def point_kernel(h, o, t, report):
    """gd_c and jac run k_solve_point"""
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, 2, seed=41, kind="tracking")
    for mode in ("gd_c", "jac"):
        p = abi.default_solve_params(mode=mode, max_steps=3, random_seed=7)
        report.read()
        b = h.solve_batch(p, seeds, params)
        assert set(report.kernels(report.read())) == {"k_solve_point"}
        a = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), mode


# ---- 7. the LDS envelope per entry point -----------------------------------------------------------------------------------------------------
def envelope_problems():
    """Three problems by the layout arithmetic of the function-level kernels (eval_lds at 64 lanes): the largest position-goal chain of at most 64 KiB,
    the smallest above it (both with n ops, T = n_goals tips, P = 3 T, V = n), and the 64-tip centipede with 63 spine joints, far beyond 160 KiB.
    Returns [(name, model, template, bytes)]."""
    best_under, best_over = None, None
    for n in range(24, 64):
        for k in range(1, 25):
            b = eval_lds(n, n, 3 * k, k, 0)
            if b <= 64 * KIB and (best_under is None or b > best_under[0]):
                best_under = (b, n, k)
            if b > 64 * KIB and (best_over is None or b < best_over[0]):
                best_over = (b, n, k)
    out = []
    for name, (b, n, k) in (("under_64k", best_under), ("over_64k", best_over)):
        m, t = position_chain(n, k)
        out.append((name, m, t, b))
    m = centipede(63, 1)
    t = ProblemTemplate(m, "body", [PoseGoal("seg62"), BalanceGoal()])
    out.append(("beyond_160k", m, t, eval_lds(63, 63, 14, 64, 0)))
    return out


def envelope(make_solver, name, model, t, bytes_, device_arrays):
    """Every entry point on one envelope problem: the oracle's results bit for bit, or BIOIK_ERR_UNSUPPORTED -- which exactly where the layout says a CU
    cannot hold the launch.  `device_arrays(a)` puts a NumPy array where bioik_stream_fitness_device can read and write it and returns (pointer, fetch)."""
    h, o = make_solver(t), orc.Oracle(t)
    n_ops, V, P, T = h.D, h.V, h.P, h.T  # (serial chains: an op per gene, no parked frames)
    assert eval_lds(n_ops, V, P, T, 0) == bytes_ or name == "beyond_160k"
    bytes_ = eval_lds(n_ops, V, P, T, 0)
    assert (name == "under_64k") == (bytes_ <= 64 * KIB) and (name == "beyond_160k") == (bytes_ > LDS_CU)
    fits = bytes_ <= LDS_CU
    exact = name != "beyond_160k"  # (the BalanceGoal's sum follows the walk: tolerances there)
    rng = np.random.default_rng(7)
    seed = random_configuration(model, rng)
    genes = random_configuration(model, rng, 40)[:, o.active_variables]
    par = t.pack_params()
    calls = {
        "eval_fk": (lambda: h.fk_genes(seed, genes), lambda: o.fk_genes(seed, genes)),
        "eval_fitness exact": (lambda: h.fitness(abi.FK_EXACT, seed, par, genes), lambda: o.fitness(abi.FK_EXACT, seed, par, genes)),
        "eval_fitness linear": (lambda: h.fitness(abi.FK_LINEAR, seed, par, genes, genes[0]), lambda: o.fitness(abi.FK_LINEAR, seed, par, genes, genes[0])),
        "eval_approximator": (lambda: h.approximator(seed, genes[0]), lambda: o.approximator(seed, genes[0])[:2]),
        "eval_check": (lambda: h.check(abi.default_solve_params(), seed, par, genes), lambda: o.check(abi.default_solve_params(), seed, par, genes)),
    }
    for what, (dev, ref) in calls.items():
        got = runs_or_refused(dev)
        assert (got is not None) == fits, (name, what)
        if got is not None:
            want = ref()
            for x, y in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
                assert np.array_equal(x, y) if exact else np.allclose(x, y, rtol=1e-10, atol=1e-12), (name, what)
    # reproduce: (4 M + 128 M) * 8 bytes -- beyond 64 KiB from 63 ops on, never beyond 160 KiB (64 ops: 67,584 B)
    parents = rng.normal(size=(2, 2, h.D)) * 0.1
    ga, gra = o.reproduce_counter(130, 0xBEEF, 1, 9, parents)
    gb, grb = h.reproduce(130, 0xBEEF, 1, 9, parents)
    assert np.array_equal(ga, gb) and np.array_equal(gra, grb)
    # the streamed fitness at 64 / 256 / 600 individuals (64 / 256 / 256 lanes; fewer where a CU would not hold them)
    for pop in (64, 256, 600):
        stream_fitness(h, o, t, pop, device_arrays, must_fit=eval_lds(n_ops, V, P, T, 0, 64) <= LDS_CU, exact=exact)
    # whole solves: the evolutionary solver (exact and linear FK) under the launcher's own LDS rules, the point solvers under their 64 KiB guard
    seeds = random_configuration(model, rng, 2)
    params = np.tile(par, (2, 1))
    for kw in ({}, {"fk_mode": abi.FK_LINEAR}):
        p = abi.default_solve_params(population=16, max_steps=2, random_seed=11, **kw)
        got = runs_or_refused(lambda: h.solve_batch(p, seeds, params))
        if got is not None:
            want = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=2)
            if exact:
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), (name, kw)
            else:
                assert np.abs(got[0] - want[0]).max() < 1e-9, (name, kw)
        elif fits:
            pytest.fail("%s: solve refused although the function level fits" % name)
    pt_fits = point_lds(n_ops, V, P, T, 0, h.D) <= 64 * KIB
    for mode in ("gd_c", "jac"):
        p = abi.default_solve_params(mode=mode, max_steps=2, random_seed=7)
        got = runs_or_refused(lambda: h.solve_batch(p, seeds, params))
        assert (got is not None) == pt_fits, (name, mode)
        if got is not None:
            want = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=2)
            if exact:
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), (name, mode)
            else:
                assert np.abs(got[0] - want[0]).max() < 1e-9, (name, mode)


def stream_fitness(h, o, t, pop, device_arrays, must_fit=True, exact=True, units=2):
    """bioik_stream_fitness_device (genes [unit][D][pop]) against the oracle's exact fitness; refused exactly when not even 64 lanes fit a CU"""
    seeds = random_configuration(t.model, np.random.default_rng(6), units)
    params = np.tile(t.pack_params(), (units, 1))
    genes = np.ascontiguousarray(np.random.default_rng(pop).uniform(-1, 1, size=(units, h.D, pop)))
    out = np.zeros((units, pop))
    arrays = [device_arrays(np.ascontiguousarray(x)) for x in (seeds, params, genes, out)]  # (kept: the device memory lives as long as its handle)
    (ds, _), (dp, _), (dg, _), (df, fetch) = arrays
    got = runs_or_refused(lambda: h.stream_fitness_device(units, pop, ds, dp, dg, df, 0) or True)
    assert (got is not None) == must_fit, pop
    if got is None:
        return
    res = fetch()
    for u in range(units):
        want, _ = o.fitness(abi.FK_EXACT, seeds[u], params[u], genes[u].T)
        assert np.array_equal(res[u], want) if exact else np.allclose(res[u], want, rtol=1e-10), (pop, u)
