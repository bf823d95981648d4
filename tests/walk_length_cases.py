"""Whole solves on serial chains of every length at which the two-joints-per-trip chain walk of the kernels compiled for one mapping can go wrong
(bioik_device.h: fk_walk_n<N, SERIAL>), shared by the host-simulator suite (tests/test_hostsim_walk_lengths.py) and the GPU suite
(tests/test_gpu_walk_lengths.py).  Every case: 4 queries, 128 children per species, 3 steps, bit for bit against the oracle.

The walk of a serial chain whose tips all hang behind its last op (DevProblem::tips_last) takes the joints behind the prefix two per trip and an odd last
one on its own; a chain with a tip in its middle takes them one per trip.  The cases:
  snake(n), n = 1, 2, 3, 4, 7, 8   odd and even counts; n = 1, 2: the pair loop runs zero times (it leaves the last joint, of an even number the last two); n = 3, 4: once
  the PR2-like right arm            a prefix of one op (the torso) and seven joints behind it
  a chain with prismatic joints     one as the first joint of a trip (op 2) and one as the second (op 5)
  a chain with a goal in its middle on the link behind op 2 (the first joint of a trip) and on the link behind op 3 (the second)
under the throughput schedule (k_solve_lean_cl64w4: both species on one wavefront, the children walked in pairs) and under the latency schedule, where
a launch of four queries runs k_solve_lean_cl4h (one child per lane and walk) and, with BIOIK_SOLVE_HELPED=0, k_solve_lean_cl4 (pairs).  Which kernel ran
is asserted from the launcher's report for every case: none of them may move to a kernel that walks its chain another way without this file noticing."""
import numpy as np

from bio_ik_amd import PoseGoal, ProblemTemplate, RobotModel, abi, pr2_like, snake
from bio_ik_amd.workload import make_queries
from oracle import orc

QUERIES, POPULATION, STEPS = 4, 128, 3

# (schedule, environment, the kernel the launcher picks for four queries of a serial chain without secondary goals at 128 children per species)
SCHEDULES = {
    "throughput": (abi.SCHEDULE_THROUGHPUT, {}, "k_solve_lean_cl64w4"),
    "latency_helped": (abi.SCHEDULE_LATENCY, {}, "k_solve_lean_cl4h"),
    "latency_pairs": (abi.SCHEDULE_LATENCY, {"BIOIK_SOLVE_HELPED": "0"}, "k_solve_lean_cl4"),
}


def sliding_chain():
    """seven joints on one chain, alternating y / z axes like snake(), of which the third and the sixth SLIDE along x.  A prismatic joint sits at its parent's
    origin (the link's length is the origin of the joint behind it), so that the joint program's folded constant `origin + value * axis` is the reference's
    frame-by-frame product bit for bit."""
    m = RobotModel("sliding_chain")
    m.add_link("base")
    prev = "base"
    for i in range(7):
        if i in (2, 5):
            m.add_link("seg%d" % i, prev, "j%d" % i, "prismatic", xyz=(0.0, 0, 0), axis=(1, 0, 0), lower=-0.05, upper=0.15, velocity=1.0)
        else:
            m.add_link("seg%d" % i, prev, "j%d" % i, "revolute", xyz=(0.1 if i else 0.0, 0, 0), axis=(0, 1, 0) if i % 2 == 0 else (0, 0, 1),
                       lower=-1.5, upper=1.5, velocity=1.0)
        prev = "seg%d" % i
    m.add_link("tip", prev, "tip_joint", "fixed", xyz=(0.1, 0, 0))
    m.add_group("snake", chain=("base", "tip"))
    return m


def _snake(n):
    return lambda: ProblemTemplate(snake(n), "snake", [PoseGoal("tip")])


# name -> (template, tips_last: every tip behind the last op, so that the walk goes two joints per trip)
CASES = {
    "snake1": (_snake(1), True),
    "snake2": (_snake(2), True),
    "snake3": (_snake(3), True),
    "snake4": (_snake(4), True),
    "snake7": (_snake(7), True),
    "snake8": (_snake(8), True),
    "right_arm": (lambda: ProblemTemplate(pr2_like(), "right_arm", [PoseGoal("r_wrist_roll_link")]), True),
    "sliding_chain": (lambda: ProblemTemplate(sliding_chain(), "snake", [PoseGoal("tip")]), True),
    # (the goals in the order the walk completes their links: the running sum of the reference, parity_cases.goal_sets_beyond_one_goal_per_tip)
    "goal_behind_op2": (lambda: ProblemTemplate(snake(6), "snake", [PoseGoal("seg2", weight=0.5), PoseGoal("tip")]), False),
    "goal_behind_op3": (lambda: ProblemTemplate(snake(6), "snake", [PoseGoal("seg3", weight=0.5), PoseGoal("tip")]), False),
}

_reference = {}


def reference(name):
    """(template, oracle, seeds, params, {schedule: the oracle's solve}) of a case: computed once, shared by every test that asks, never written to.  The oracle
    must be in trig mode 1 (the caller's fixture).  Before anything is compared with them the oracle's own answers are checked: finite, every query stepped
    its budget or passed, and the search moved (the best fitness of a query is below that of its seed)."""
    if name not in _reference:
        t = CASES[name][0]()
        o = orc.Oracle(t)
        seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, QUERIES, seed=7)
        want, by_schedule = {}, {}  # (the oracle knows no lane mapping: one solve per schedule value)
        for key, (schedule, _, _) in SCHEDULES.items():
            if schedule not in by_schedule:
                p = abi.default_solve_params(population=POPULATION, max_steps=STEPS, random_seed=11, schedule=schedule)
                sol, fit, suc, steps = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=4)
                assert np.isfinite(sol).all() and np.isfinite(fit).all()
                assert np.all((steps == STEPS) | (suc == 1)) and steps.min() >= 1
                at_seed, _ = o.fitness(abi.FK_EXACT, seeds[0], params[0], seeds[:1, o.active_variables])
                assert fit[0] < at_seed[0]
                for a in (sol, fit, suc, steps):
                    a.setflags(write=False)
                by_schedule[schedule] = (sol, fit, suc, steps)
            want[key] = by_schedule[schedule]
        seeds.setflags(write=False), params.setflags(write=False)
        _reference[name] = (t, o, seeds, params, want)
    return _reference[name]


def solve(name, key, make_solver, report, monkeypatch):
    """the case under one schedule on the solver of `make_solver`: bit for bit the oracle's, on the kernel SCHEDULES names; returns the solve"""
    t, o, seeds, params, want = reference(name)
    schedule, env, kernel = SCHEDULES[key]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = make_solver(t)
    assert (h.D, h.T) == (o.D, o.T)
    p = abi.default_solve_params(population=POPULATION, max_steps=STEPS, random_seed=11, schedule=schedule)
    report.read()
    got = h.solve_batch(p, seeds, params)
    ran = set(report.kernels(report.read()))
    for k in env:
        monkeypatch.delenv(k)
    assert ran == {kernel}, (name, key, ran)
    for a, b, what in zip(want[key], got, ("solutions", "fitness", "success", "steps")):
        assert np.array_equal(a, b), "%s under %s: %s differ" % (name, key, what)
    return got
