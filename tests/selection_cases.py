"""Whole solves that take the elitist selection and the winners' copy of a generation (solve_select_and_copy, bioik_kernels.h) through every path of the form
compiled for the dense mapping (k_solve_lean_cl64w4: both species of a query on the halves of one wavefront, a lane's keys in registers), shared by the
host-simulator suite (tests/test_hostsim_dense_selection.py) and the GPU suite (tests/test_gpu_dense_selection.py).  Every case: 1 to 4 queries, 1 to 4 steps
under the throughput schedule, bit for bit against the oracle (solutions, fitness, success, steps).

The cases are the smallest shapes at which that code can go wrong:
  populations     128, 131, 160, 200, 255, 256 children: 4, 5, 5, 7, 8, 8 keys per lane on a group of 32 -- the form of four keys and the form of eight, with tails
                  where only some lanes hold a last key (padding) and where every lane holds all eight
  chains          the 7-joint arm (8 ops: both winners are copied at once, sixteen lanes each); a serial chain of 20 ops (one winner per pass, the second
                  winner first); 34 ops of which three are fixed (`d31_fixed` of line_search_cases.py: a lane copies ops k and k + 32, ops that are no genes)
  keys            BIOIK_SOLVE_SORT_KEY_DROP = 10, 36, 50: the mask of the dropped bits inside the low word, across both words and deep in the high word; keys
                  that give up 50 bits (classes of a quarter of a value) send every generation of a first step through the exact path behind the doubt test, for
                  four and for eight keys per lane and for a winner per pass (counted below; at 36 bits, classes of 1.5e-5, the first steps meet none)
  ties            joints without any range (every child of a generation is the same genotype: every fitness ties and position decides), against the oracle;
                  and the coarse-fitness switch of the parity suites (BIOIK_SOLVE_TIE_TEST_BITS: most generations have several best children) -- the oracle knows
                  no such switch, so there the dense kernel is held against the library's latency mapping under the same switch, bit for bit
  parents         every other query starts AT its goal (`at_goal`): the parents are the best of every generation and stay -- the copy of a parent
  hand-over       a solve cut after its first step (BIOIK_SOLVE_TWO_PHASE=1) and one whose units leave at their own step (BIOIK_SOLVE_DRAIN_TEST): what the dense
                  launch leaves must be what k_solve_lean_cl4h continues from

Which situations the ORACLE's run shows is counted, not assumed: situations() restates the generations of a query's first step on the oracle's own functions
(its reproduction, its exact fitness, the reference's selection sort), checks the restated elites against the oracle's solver after one step, and counts per
generation and species whether a child took first place, a child took second place, both parents stayed, and whether the keys of that generation put the
selection in doubt (two or more children share the upper bits of the runner-up's key: the exact path).  The tests assert that every one occurred."""
import numpy as np

import line_search_cases as ls
from bio_ik_amd import PoseGoal, ProblemTemplate, abi, pr2_like, snake
from bio_ik_amd.workload import make_queries
from oracle import orc

KERNEL = "k_solve_lean_cl64w4"
SUCCESSOR = "k_solve_lean_cl4h"

CHAINS = {
    "arm": lambda: ProblemTemplate(pr2_like(), "right_arm", [PoseGoal("r_wrist_roll_link")]),  # 8 ops, 7 genes
    "d20": lambda: ProblemTemplate(snake(20), "snake", [PoseGoal("tip")]),                      # more than 16 ops: one winner per pass
    "d31_fixed": ls.CASES["d31_fixed"][0],                                                       # 34 ops, 31 genes: ops k and k + 32 of a lane
    "no_range": lambda: ProblemTemplate(snake(4, limit=0.0), "snake", [PoseGoal("tip")]),        # every fitness of a generation is the same number
}
SHAPES = {"arm": (8, 7, 1), "d20": (20, 20, 1), "d31_fixed": (34, 31, 1), "no_range": (4, 4, 1)}  # (ops, genes, tips)


def _case(chain, pop, n=2, steps=2, env=None, mode=None, kernels=(KERNEL,), against="oracle", at_goal=False):
    return dict(chain=chain, pop=pop, n=n, steps=steps, env=env or {}, mode=mode, kernels=set(kernels), against=against, at_goal=at_goal)


CASES = {
    # populations: 4, 5, 5, 7, 8, 8 keys per lane
    "pop128": _case("arm", 128, n=4, steps=3),
    "pop131": _case("arm", 131),
    "pop160": _case("arm", 160),
    "pop200": _case("arm", 200),
    "pop255": _case("arm", 255),
    "pop256": _case("arm", 256),
    # chains: one winner per pass; the second op of a lane
    "d20_pop128": _case("d20", 128),
    "d20_pop200": _case("d20", 200, n=1),
    "d31_fixed_pop128": _case("d31_fixed", 128),
    "d31_fixed_pop131": _case("d31_fixed", 131, n=1),
    # keys that give up more bits: the exact path behind the doubt test
    "drop10": _case("arm", 128, n=4, steps=2, env={"BIOIK_SOLVE_SORT_KEY_DROP": "10"}),
    "drop36": _case("arm", 128, n=4, steps=2, env={"BIOIK_SOLVE_SORT_KEY_DROP": "36"}),
    "drop50": _case("arm", 128, n=4, steps=2, env={"BIOIK_SOLVE_SORT_KEY_DROP": "50"}),
    "drop36_pop200": _case("arm", 200, env={"BIOIK_SOLVE_SORT_KEY_DROP": "36"}),
    "drop50_pop255": _case("arm", 255, env={"BIOIK_SOLVE_SORT_KEY_DROP": "50"}),
    "drop50_d20": _case("d20", 128, env={"BIOIK_SOLVE_SORT_KEY_DROP": "50"}),
    # ties: position decides
    "no_range_pop128": _case("no_range", 128),
    "no_range_pop200": _case("no_range", 200),
    "coarse46": _case("arm", 128, n=4, steps=3, env={"BIOIK_SOLVE_TIE_TEST_BITS": "46"}, mode="bio2", against="latency"),
    "coarse50": _case("arm", 128, n=4, steps=3, env={"BIOIK_SOLVE_TIE_TEST_BITS": "50"}, mode="bio2", against="latency"),
    "coarse50_pop200": _case("arm", 200, env={"BIOIK_SOLVE_TIE_TEST_BITS": "50"}, mode="bio2", against="latency"),
    # the parents stay: odd queries start at their goal
    "at_goal": _case("arm", 128, n=4, steps=2, at_goal=True),
    "at_goal_d20_pop160": _case("d20", 160, at_goal=True),
    # hand-over: the state the dense launch leaves for k_solve_lean_cl4h
    "two_phase": _case("arm", 128, n=4, steps=3, env={"BIOIK_SOLVE_TWO_PHASE": "1"}, kernels=(KERNEL, SUCCESSOR)),
    "drain": _case("arm", 128, n=4, steps=4, env={"BIOIK_SOLVE_DRAIN_TEST": "3"}, kernels=(KERNEL, SUCCESSOR)),
}


def _params(case, schedule=abi.SCHEDULE_THROUGHPUT, **kw):
    if case["mode"]:
        kw["mode"] = case["mode"]
    return abi.default_solve_params(population=case["pop"], max_steps=case["steps"], random_seed=11, schedule=schedule, **kw)


_templates, _reference = {}, {}


def problem(chain):
    """(template, oracle) of a chain: built once"""
    if chain not in _templates:
        t = CHAINS[chain]()
        _templates[chain] = (t, orc.Oracle(t))
    return _templates[chain]


def reference(name):
    """(template, oracle, seeds, params, the oracle's solve or None) of a case: computed once, shared, never written to.  The oracle must be in trig mode 1
    (the caller's fixture)."""
    if name not in _reference:
        case = CASES[name]
        t, o = problem(case["chain"])
        seeds, params, targets = make_queries(t, o.active_variables, o.fk_genes, case["n"], seed=7)
        if case["at_goal"]:
            seeds[1::2, np.asarray(o.active_variables)] = targets[1::2]
        seeds.setflags(write=False), params.setflags(write=False)
        want = None
        if case["against"] == "oracle":
            want = o.solve_batch(_params(case), orc.RNG_COUNTER, seeds, params, n_threads=1)
            for a in want:
                a.setflags(write=False)
        _reference[name] = (t, o, seeds, params, want)
    return _reference[name]


def solve(name, make_solver, report, monkeypatch):
    """the case on the solver of `make_solver`: on the dense kernel (and, after a hand-over, its successor), bit for bit the oracle's -- or, under the
    coarse-fitness switch, the same library's latency mapping under the same switch; returns the solve"""
    case = CASES[name]
    t, o, seeds, params, want = reference(name)
    h = make_solver(t)
    assert (h.D, h.T) == (o.D, o.T) == SHAPES[case["chain"]][1:]
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    try:
        report.read()
        got = h.solve_batch(_params(case), seeds, params)
        text = report.read()
        assert set(report.kernels(text)) == case["kernels"], (name, report.kernels(text))
        assert report.shape(text)[:3] == SHAPES[case["chain"]], (name, report.shape(text))
        if want is None:
            want = h.solve_batch(_params(case, schedule=abi.SCHEDULE_LATENCY), seeds, params)
            assert KERNEL not in report.kernels(report.read()), name
    finally:
        for k in case["env"]:
            monkeypatch.delenv(k)
    for a, b, what in zip(want, got, ("solutions", "fitness", "success", "steps")):
        assert np.array_equal(a, b), "%s: %s differ" % (name, what)
    return got


def coarse_values_change_the_search(make_solver, monkeypatch):
    """the coarse-fitness cases are there for ties: with the switch the search must go elsewhere than without it"""
    case = CASES["coarse50"]
    t, o, seeds, params, _ = reference("coarse50")
    h = make_solver(t)
    plain = h.solve_batch(_params(case), seeds, params)
    monkeypatch.setenv("BIOIK_SOLVE_TIE_TEST_BITS", "50")
    try:
        coarse = h.solve_batch(_params(case), seeds, params)
    finally:
        monkeypatch.delenv("BIOIK_SOLVE_TIE_TEST_BITS")
    return not np.array_equal(plain[0], coarse[0])


def situations(name):
    """What the selection of every generation of the FIRST step of every query's two species meets in the oracle's run, restated on the oracle's functions.
    Returns a dict of counts over the case's queries: generations, child_first, child_second, parents_stay, doubt (the keys of the case's
    BIOIK_SOLVE_SORT_KEY_DROP put the runner-up in doubt), ties (the least fitness of the children is shared by two or more of them).  The restated SECOND
    elite of each species -- the first is what the line search behind the generations edits -- is checked against the oracle's own solver after one step, bit for bit:
    eight generations' winners in a row."""
    case = CASES[name]
    t, o, seeds, params, _ = reference(name)
    p = abi.default_solve_params(population=case["pop"], max_steps=case["steps"], random_seed=11, schedule=abi.SCHEDULE_THROUGHPUT, no_wipeout=1)  # (the wipe-out follows the generations: without it the state shows both species' elites)
    act = np.asarray(o.active_variables)
    D = o.D
    drop = int(case["env"].get("BIOIK_SOLVE_SORT_KEY_DROP", "10"))
    low = np.uint64((1 << drop) - 1)
    count = dict(generations=0, child_first=0, child_second=0, parents_stay=0, doubt=0, ties=0)
    for k in range(seeds.shape[0]):
        seed, par = seeds[k], params[k]
        key = orc.query_key(p.random_seed, k, 0)
        elites = []
        for s in (0, 1):
            pop = np.zeros((2, 2, D))
            pop[:, 0, :] = seed[act]
            for gen in range(8):  # ik_evolution_2.cpp:348-431 on the oracle's reproduction and exact fitness
                cg, cd = o.reproduce_counter(p.population, key, s, gen, pop)
                genes, grads = np.concatenate([pop[:, 0, :], cg]), np.concatenate([pop[:, 1, :], cd])
                fit = o.fitness(abi.FK_EXACT, seed, par, genes)[0]
                idx = list(range(len(fit)))
                for i in range(2):  # the reference's selection sort, two places of it (:410-423)
                    jmin = i
                    for j in range(i + 1, len(idx)):
                        if fit[idx[j]] < fit[idx[jmin]]:
                            jmin = j
                    idx[i], idx[jmin] = idx[jmin], idx[i]
                count["generations"] += 1
                count["child_first"] += idx[0] >= 2
                count["child_second"] += idx[1] >= 2
                count["parents_stay"] += idx[0] < 2 and idx[1] < 2
                # the children's keys (sort_key): the fitness's upper bits and the position; in doubt: a second child shares the runner-up's upper bits
                child = np.ascontiguousarray(fit[2:])
                keys = np.sort((child.view(np.uint64) & ~low) | (np.arange(len(child), dtype=np.uint64) + np.uint64(2)))
                count["doubt"] += int(np.count_nonzero((keys ^ keys[1]) <= low)) >= 2
                count["ties"] += int(np.count_nonzero(child == child.min())) >= 2
                pop = np.stack([np.stack([genes[idx[i]], grads[idx[i]]]) for i in range(2)])
            elites.append(pop[1, 0].copy())
        sv = o.solver(p, orc.RNG_COUNTER, key, seed, par)
        sv.step()
        got = sv.state()[0][:, 1, 0, :]
        for x in elites:
            assert any(np.array_equal(got[r], x) for r in range(2)), "the restated first step is not the oracle's (%s, query %d)" % (name, k)
    return count


# the cases whose first steps are counted (every chain, both forms of the keys, the three widths of the keys, true ties) and what their sum must show
COUNTED = ("pop128", "pop200", "d20_pop128", "d31_fixed_pop128", "drop36", "drop50", "drop50_pop255", "drop50_d20", "no_range_pop128", "at_goal", "at_goal_d20_pop160")
