"""Whole solves that take the memetic line search (solve_memetic, bioik_kernels.h) through every path of the form compiled for the dense mapping
(k_solve_lean_cl64w4: both species of a query on the halves of one wavefront), shared by the host-simulator suite (tests/test_hostsim_line_search.py) and
the GPU suite (tests/test_gpu_line_search.py).  Every case: QUERIES queries, 128 children per species, STEPS steps under the throughput schedule, both
line searches ('q': bio2_memetic, 'l': bio2_memetic_l), bit for bit against the oracle (solutions, fitness, success, steps).

The cases are the smallest shapes at which that code can go wrong:
  chain lengths   serial chains of D = 1, 2, 3, 5, 7, 8, 9, 31 genes: the chains' loop of four ops per trip runs 0, 1, 2 or 7 times and its remainder loop 0 ... 3
                  times; ops that are no genes (fixed joints: their value is the seed's) in front of, between and behind the genes, so that masked ops sit inside
                  the chains (`d3_fixed`, `arm`); 34 ops for 31 genes, the second op of a lane (`d31_fixed`: ops 32, 33)
  tips            a chain with a second tip in its middle (`two_tips`: T = 2, sixteen component lanes)
  bounds          continuous joints without limits between limited ones (`continuous`: a clip range of +-DBL_MAX beside finite ones), and the rule for candidates
                  without bound (`unbounded`: a goal 1e7 m and more away, whose support values can lie on a straight line exactly -- a quadratic step of v / 0 on a
                  joint without limits; quirks Q5 / Q7 of DESIGN.md section 3)
and every case's queries are of three kinds (queries()): reachable poses far from the seed (many candidates accepted, the cap of eight iterations), seeds at
joint limits (clipped candidates), the seed's own pose as the target (nothing to gain: the search stops at once -- the linear search on a step that is not a
number).  `flat` is a joint that does not move its goal: three equal support values, a step that is not a number in both searches.

Which of these situations the ORACLE's run shows is counted, not assumed: situations() restates the first step of a query's two species on the oracle's own
functions (its reproduction, its exact fitness, its approximator tables, its goal fitness on frames), checks the restated elites against the oracle's solver
after one step, and reports per species how many candidates were accepted and why the search stopped; candidates without bound are also counted by the
oracle's own counter over its whole solve (UNBOUNDED_MET).  The tests assert the counts (EXPECTED_TOTAL), so that a drift of the inputs cannot empty a case
silently."""
import numpy as np

from bio_ik_amd import PoseGoal, PositionGoal, ProblemTemplate, RobotModel, abi, pr2_like, snake
from bio_ik_amd.workload import make_queries
from oracle import orc

QUERIES, POPULATION, STEPS = 12, 128, 4
KERNEL = "k_solve_lean_cl64w4"
MODES = {"q": "bio2_memetic", "l": "bio2_memetic_l"}


def continuous_chain():
    """five joints on one chain, the second and the fourth CONTINUOUS (no limits: the clip range is +-DBL_MAX)"""
    m = RobotModel("continuous_chain")
    m.add_link("base")
    prev = "base"
    for i in range(5):
        kw = {} if i in (1, 3) else {"lower": -1.5, "upper": 1.5}
        m.add_link("seg%d" % i, prev, "j%d" % i, "continuous" if i in (1, 3) else "revolute", xyz=(0.1 if i else 0.0, 0, 0), axis=(0, 1, 0) if i % 2 == 0 else (0, 0, 1),
                   velocity=1.0, **kw)
        prev = "seg%d" % i
    m.add_link("tip", prev, "tip_joint", "fixed", xyz=(0.1, 0, 0))
    m.add_group("snake", chain=("base", "tip"))
    return m


def flat_chain():
    """one joint that turns its link about the link's own origin, under a goal on that link's POSITION: the fitness does not depend on the gene"""
    m = RobotModel("flat_chain")
    m.add_link("base")
    m.add_link("seg0", "base", "j0", "revolute", xyz=(0.2, 0.1, 0.0), axis=(0, 0, 1), lower=-1.5, upper=1.5, velocity=1.0)
    m.add_group("snake", joints=["j0"], tips=["seg0"])
    return m


def far_chain():
    """three joints on one chain, the first and the last continuous, under a goal on the tip's POSITION that queries() puts 1e7 m and more away: the fitness
    is ~1e15 and its changes along the gradient are a few units in its last place, so that the three support values of a line search can lie on a straight line
    exactly -- a quadratic step of v / 0 -- and a joint without limits is sent to the end of its clip range"""
    m = RobotModel("far_chain")
    m.add_link("base")
    prev = "base"
    for i in range(3):
        kw = {"lower": -1.5, "upper": 1.5} if i == 1 else {}
        m.add_link("seg%d" % i, prev, "j%d" % i, "revolute" if i == 1 else "continuous", xyz=(0.1 if i else 0.0, 0, 0), axis=(0, 1, 0) if i % 2 == 0 else (0, 0, 1),
                   velocity=1.0, **kw)
        prev = "seg%d" % i
    m.add_link("tip", prev, "tip_joint", "fixed", xyz=(0.1, 0, 0))
    m.add_group("snake", chain=("base", "tip"))
    return m


FAR_TARGETS = ((2e7, 1e7, 5e6), (3e8, -1e8, 2e8))  # (even queries, odd queries of the case `unbounded`)


def _snake(n, fixed=()):
    return lambda: ProblemTemplate(snake(n), "snake", [PoseGoal("tip")], fixed_joints=["j%d" % k for k in fixed])


# name -> (template, (ops, genes, tips) of its joint program)
CASES = {
    "d1": (_snake(1), (1, 1, 1)),
    "d2": (_snake(2), (2, 2, 1)),
    "d3_fixed": (_snake(6, fixed=(0, 2, 5)), (6, 3, 1)),  # fixed ops in front of, between and behind the genes
    "d5": (_snake(5), (5, 5, 1)),
    "arm": (lambda: ProblemTemplate(pr2_like(), "right_arm", [PoseGoal("r_wrist_roll_link")]), (8, 7, 1)),  # the torso in front of seven genes
    "d8": (_snake(8), (8, 8, 1)),
    "d9": (_snake(9), (9, 9, 1)),
    "d31": (_snake(31), (31, 31, 1)),
    "d31_fixed": (_snake(34, fixed=(3, 17, 33)), (34, 31, 1)),  # ops 32 and 33: the second op of lanes 0 and 1
    "two_tips": (lambda: ProblemTemplate(snake(6), "snake", [PoseGoal("seg2", weight=0.5), PoseGoal("tip")]), (6, 6, 2)),
    "continuous": (lambda: ProblemTemplate(continuous_chain(), "snake", [PoseGoal("tip")]), (5, 5, 1)),
    "flat": (lambda: ProblemTemplate(flat_chain(), "snake", [PositionGoal("seg0", (0.3, 0.2, 0.1))]), (1, 1, 1)),
    "unbounded": (lambda: ProblemTemplate(far_chain(), "snake", [PositionGoal("tip")]), (3, 3, 1)),
}


def queries(t, o, n=QUERIES, seed=7):
    """n queries of three kinds, in turn: (0) a reachable pose far from the seed, (1) the same with every other gene of the seed at a joint limit,
    (2) the seed's own pose as the target"""
    seeds, params, targets = make_queries(t, o.active_variables, o.fk_genes, n, seed=seed)
    act = np.asarray(o.active_variables)
    lo, hi = np.asarray(t.model.var_min)[act], np.asarray(t.model.var_max)[act]
    for k in range(n):
        if k % 3 == 1:
            g = seeds[k, act].copy()
            for i in range(0, len(act), 2):
                lim = lo[i] if (i // 2 + k) % 2 == 0 else hi[i]
                if np.isfinite(lim) and abs(lim) < 1e6:
                    g[i] = lim
            seeds[k, act] = g
        elif k % 3 == 2:
            seeds[k, act] = targets[k]
    if t.model.name == "far_chain":
        for k in range(n):
            params[k, 0:3] = FAR_TARGETS[k % 2]
    return seeds, params


def _solve_params(mode, **kw):
    return abi.default_solve_params(population=POPULATION, max_steps=STEPS, random_seed=11, mode=MODES[mode], schedule=abi.SCHEDULE_THROUGHPUT, **kw)


def situations(t, o, seeds, params, mode):
    """What the line searches of the FIRST step of every query's two species do in the oracle's run, restated on the oracle's functions: per species the
    candidates accepted and the reason the search stopped.  Returns a dict of counts over the batch.  The restated elites are checked against the oracle's own
    solver after one step (to 1e-9: the restatement adds `delta * dp` where the oracle fuses)."""
    p = _solve_params(mode, no_wipeout=1)  # (the wipe-out follows the line search: without it the solver's state shows both species' elites)
    act = np.asarray(o.active_variables)
    D = o.D
    info = o.robot_info()[act]
    bound = orc.candidate_bound()
    count = dict(searches=0, accepted=0, cap=0, rejected=0, nan=0, unbounded=0, clipped=0, out_of_step=0, no_candidate_accepted=0)
    for k in range(seeds.shape[0]):
        seed, par = seeds[k], params[k]
        key = orc.query_key(p.random_seed, k, 0)
        elites, iters = [], []
        for s in (0, 1):
            pop = np.zeros((2, 2, D))
            pop[:, 0, :] = seed[act]
            for gen in range(8):  # ik_evolution_2.cpp:348-431 on the oracle's reproduction and exact fitness
                cg, cd = o.reproduce_counter(p.population, key, s, gen, pop)
                genes, grads = np.concatenate([pop[:, 0, :], cg]), np.concatenate([pop[:, 1, :], cd])
                fit = o.fitness(abi.FK_EXACT, seed, par, genes)[0]
                idx = list(range(len(fit)))
                for i in range(2):
                    jmin = i
                    for j in range(i + 1, len(idx)):
                        if fit[idx[j]] < fit[idx[jmin]]:
                            jmin = j
                    idx[i], idx[jmin] = idx[jmin], idx[i]
                pop = np.stack([np.stack([genes[idx[i]], grads[idx[i]]]) for i in range(2)])
            base = pop[0, 0].copy()
            x = base.copy()
            _, deltas, _ = o.approximator(seed, base)
            dp = 0.0000001
            if orc.counter_uniform(key, 0, (0 << 4) | (s << 3) | 2) < 0.5:
                dp = -dp

            def value(g):
                return o.fitness_frames(seed, par, o.approx_eval(seed, base, g)[0], g)

            count["searches"] += 1
            n_acc, it = 0, 0
            for it in range(1, 9):  # :436-570
                fr = o.approx_eval(seed, base, x)[0]
                f2p, sec = o.fitness_frames(seed, par, fr, x)
                fa = f2p + sec
                grad = np.zeros(D)
                for i in range(D):
                    xi = x.copy()
                    xi[i] += dp
                    grad[i] = sum(o.fitness_frames(seed, par, fr + deltas[:, i, :] * dp, xi)) - fa
                total = dp * dp
                for i in range(D):
                    total += abs(grad[i])
                grad = grad * (1.0 / total * dp)
                f1, f3 = sum(value(x - grad)), sum(value(x + grad))
                with np.errstate(all="ignore"):
                    if mode == "q":
                        v1, v2 = np.float64(fa - f1), np.float64(f3 - fa)
                        raw = x + grad * ((v1 + v2) * 0.5 / (v1 - v2))
                    else:
                        raw = x - grad * (np.float64(fa) / np.float64((f3 - f1) * 0.5))
                if np.isnan(raw).any():
                    count["nan"] += 1
                    break
                cand = np.minimum(np.maximum(raw, info[:, 0]), info[:, 1])
                if (np.abs(cand) >= bound).any():
                    count["unbounded"] += 1
                    break
                if (cand != raw).any():
                    count["clipped"] += 1
                if value(cand)[0] < f2p:
                    x = cand
                    n_acc += 1
                    if it == 8:
                        count["cap"] += 1
                else:
                    count["rejected"] += 1
                    break
            count["accepted"] += n_acc
            count["no_candidate_accepted"] += n_acc == 0
            elites.append(x)
            iters.append(it)
        count["out_of_step"] += iters[0] != iters[1]
        sv = o.solver(p, orc.RNG_COUNTER, key, seed, par)
        sv.step()
        got = sv.state()[0][:, 0, 0, :]
        for x in elites:
            assert min(np.abs(got[r] - x).max() for r in range(2)) < 1e-9, "the restated first step is not the oracle's (query %d)" % k
    return count


# what the oracle's run must show at the least, per line search ('q', 'l'), summed over the cases (asserted by test_the_situations_are_met) ...
EXPECTED_TOTAL = {  # (about half of what the oracle's run of these inputs shows: 1208 / 527 candidates accepted, 121 / 15 searches at the cap, ...)
    "q": {"accepted": 600, "cap": 60, "rejected": 80, "nan": 24, "unbounded": 1, "clipped": 380, "out_of_step": 12, "no_candidate_accepted": 60},
    "l": {"accepted": 260, "cap": 7, "rejected": 85, "nan": 60, "clipped": 220, "out_of_step": 23, "no_candidate_accepted": 65},
}

_reference = {}
UNBOUNDED_MET = {}  # (case, line search) -> candidates with a gene of magnitude candidate_bound() or more that the ORACLE'S whole solve met and dropped (its own counter)


def reference(name, mode):
    """(template, oracle, seeds, params, the oracle's solve) of a case under one line search: computed once, shared, never written to.  The oracle must be in
    trig mode 1 (the caller's fixture)."""
    if (name, mode) not in _reference:
        if name not in _reference:
            t = CASES[name][0]()
            o = orc.Oracle(t)
            seeds, params = queries(t, o)
            seeds.setflags(write=False), params.setflags(write=False)
            _reference[name] = (t, o, seeds, params)
        t, o, seeds, params = _reference[name]
        met = orc.unbounded_candidates()
        want = o.solve_batch(_solve_params(mode), orc.RNG_COUNTER, seeds, params, n_threads=1)
        UNBOUNDED_MET[(name, mode)] = orc.unbounded_candidates() - met
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.abs(want[0]).max() < orc.candidate_bound()
        assert np.all((want[3] == STEPS) | (want[2] == 1))
        for a in want:
            a.setflags(write=False)
        _reference[(name, mode)] = (t, o, seeds, params, want)
    return _reference[(name, mode)]


def solve(name, mode, make_solver, report):
    """the case on the solver of `make_solver`: on the dense kernel, bit for bit the oracle's; returns the solve"""
    t, o, seeds, params, want = reference(name, mode)
    h = make_solver(t)
    assert (h.D, h.T) == (o.D, o.T) == CASES[name][1][1:]
    report.read()
    got = h.solve_batch(_solve_params(mode), seeds, params)
    text = report.read()
    assert set(report.kernels(text)) == {KERNEL}, (name, mode, report.kernels(text))
    assert report.shape(text)[:3] == CASES[name][1], (name, report.shape(text))
    for a, b, what in zip(want, got, ("solutions", "fitness", "success", "steps")):
        assert np.array_equal(a, b), "%s, line search '%s': %s differ" % (name, mode, what)
    return got
