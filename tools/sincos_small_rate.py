#!/usr/bin/env python3
"""How often can a whole wavefront of a chain walk take the small-half-angle sincos (bioik_sincos.h: bioik_sincos_small; bioik_platform.h: p_sincos_n)?
Counted on the CPU with the oracle's stepping solver, before any GPU time is spent on it.

    python tools/sincos_small_rate.py [--queries 96] [--configs c2,c3,c4]

The queries are bench.py's (make_queries(seed=0xB101C), its templates and parameters: C2 the PR2-like right arm, 128 children, 64 steps; C3 both arms and the
torso with MinimalDisplacement, 128 children, 128 steps; C4 the 31-joint snake, 512 children, 32 steps).  Each query is stepped with the counter generator until
it succeeds or its budget ends; at every step the parents of both species (OracleSolver.state()) are handed to Oracle.reproduce_counter, which returns the
children the solver breeds from them (rows 2 ... of the population: rows 0, 1 are the elites), and the half angles gene / 2 of every revolute gene are held
against BIOIK_SINCOS_SMALL in the groups in which one trip of the device's walk sees them:

    C2 (k_solve_lean_cl64w4) and C4 (k_solve_lean_cl4 at one species per wavefront: the same figure with one species' 128 children per trip of 64 lanes x 2)
        a trip walks children r0 ... r0 + 63 of BOTH species together, two per lane (r, r + 32 of a species on a half-wavefront): one vote per joint over 128 children
    C3 (k_solve_lean_clj4) the children of both species as one list over the 64 lanes, two per lane: votes over 128 consecutive items of that list

What this is NOT: (1) the children are bred once per STEP, from the parents the step starts with -- the sixteen generations inside a step breed from parents
that have moved on, which the stepping solver does not show; the first generation stands for them.  (2) reproduce_counter is called with the query's key and
the step as the generation number, not with the solver's own counter: the same distribution of children, not the same children.  (3) with a secondary goal
(C3, C4) the device walks a pre-selected, sorted prefix of the children; here they are taken in row order, all of them.  For C4 none of this matters: every
gene is clipped to its limits of +-1.5 rad, a half angle of at most 0.75 < BIOIK_SINCOS_SMALL.

Per gene (chain order) and overall: the wave-level rate (every child of the group small: the vote passes), the per-lane rate (a child's own half angle is
small) and the rate at which every child of the group has the SAME multiple of pi / 2 (fn = rint(h * 2 / pi)), zero or not.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bio_ik_amd import AvoidJointLimitsGoal, MinimalDisplacementGoal, PoseGoal, ProblemTemplate, abi, pr2_like, snake  # noqa: E402
from bio_ik_amd.workload import make_queries  # noqa: E402
from oracle import orc  # noqa: E402

SMALL = 0.78  # BIOIK_SINCOS_SMALL (bio_ik_amd/csrc/bioik_sincos.h; tests/sincos_small_cases.py holds the library's value against its conditions)
INVPIO2 = 6.36619772367581382433e-01

CONFIGS = {
    "c2": (lambda: ProblemTemplate(pr2_like(), "right_arm", [PoseGoal("r_wrist_roll_link")]), 128, 64),
    "c3": (lambda: ProblemTemplate(pr2_like(), "all", [PoseGoal("r_wrist_roll_link"), PoseGoal("l_wrist_roll_link"), MinimalDisplacementGoal()]), 128, 128),
    "c4": (lambda: ProblemTemplate(snake(31), "snake", [PoseGoal("tip"), AvoidJointLimitsGoal()]), 512, 32),
}


def revolute_genes(template, active_variables):
    m = template.model
    kind = {m.joint_first_variable[l]: m.joint_type[l] for l in range(len(m.link_names)) if m.joint_first_variable[l] >= 0}
    return np.array([kind[int(v)] == abi.JOINT_REVOLUTE for v in active_variables])


def groups(name, c0, c1):
    """the children (rows [n, D] of species 0 and 1) in the groups one vote covers: a list of [m, D] arrays"""
    if name == "c3":
        both = np.concatenate([c0, c1])
        return [both[i:i + 128] for i in range(0, len(both), 128)]
    return [np.concatenate([c0[i:i + 64], c1[i:i + 64]]) for i in range(0, len(c0), 64)]


def count(name, n_queries):
    make, pop, max_steps = CONFIGS[name]
    t = make()
    o = orc.Oracle(t)
    rev = revolute_genes(t, o.active_variables)
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, 4096, seed=0xB101C)
    p = abi.default_solve_params(population=pop, max_steps=max_steps, random_seed=1)
    D = o.D
    votes = np.zeros(D)
    passed = np.zeros(D)
    same = np.zeros(D)
    lanes = np.zeros(D)
    lanes_small = np.zeros(D)
    samples = 0
    for q in range(n_queries):
        key = orc.query_key(p.random_seed, q, 0)
        s = o.solver(p, orc.RNG_COUNTER, key, seeds[q], params[q])
        for step in range(max_steps):
            g = s.state()[0]  # [species][parent][genes, gradients][D]
            kids = [o.reproduce_counter(pop, key, sp, step, g[sp])[0][2:] for sp in (0, 1)]
            samples += 1
            for grp in groups(name, kids[0], kids[1]):
                h = grp * 0.5
                small = np.abs(h) <= SMALL
                fn = np.rint(h * INVPIO2)
                votes += 1
                passed += small.all(axis=0)
                same += (fn == fn[0]).all(axis=0)
                lanes += len(grp)
                lanes_small += small.sum(axis=0)
            s.step()
            if s.check()[0]:
                break
    print("%s: %d queries, %d step samples, %d children per species, %d genes of which %d revolute" % (name, n_queries, samples, pop - 2, D, int(rev.sum())))
    print("  gene (chain order)      " + " ".join("%6d" % k for k in range(D)))
    print("  revolute                " + " ".join("%6s" % ("yes" if r else "no") for r in rev))
    for label, a, b in (("wave-level small", passed, votes), ("per-lane small", lanes_small, lanes), ("same fn in every lane", same, votes)):
        r = a / b
        print("  %-23s " % label + " ".join("%6.3f" % x for x in r) + "   mean over the revolute genes %.3f" % r[rev].mean())
    return (passed / votes)[rev].mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=96)
    ap.add_argument("--configs", default="c2,c3,c4")
    a = ap.parse_args()
    orc.set_trig_mode(1)
    print("BIOIK_SINCOS_SMALL = %.2f; children bred by Oracle.reproduce_counter from the parents of every step (see the head of tools/sincos_small_rate.py for what that leaves out)" % SMALL)
    for name in a.configs.split(","):
        count(name, a.queries if name == "c2" else max(4, a.queries // 8))


if __name__ == "__main__":
    main()
