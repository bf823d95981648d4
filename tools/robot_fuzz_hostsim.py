"""Robot soak WITHOUT a GPU: random kinematic TREES -- revolute, continuous, prismatic and fixed joints anywhere, rotated origins, oblique axes, mimic joints,
branches at any depth, tips on inner links, on fixed links and off the root, fixed_joints -- with goals listed in walk order, in the host simulator
(tests/hostsim) against the CPU oracle.  Twice per robot: the unfolded joint program (BIOIK_COMPILE_EXACT=1, bioik_compile.cpp), where FK, fitness, tables,
success test and a whole solve must be the oracle's bit for bit on ANY robot, and the default (folded) program, which must agree to rounding (1e-12).
ROBOT_FUZZ_GRADIENT=1: every third robot is solved by a point solver of the gradient family (gd / gd_r / gd_c) instead; ROBOT_FUZZ_BIG=1: 12 - 30 links, up to six tips; ROBOT_FUZZ_PLAIN=1: trees whose default program folds exactly (unrotated origins, no prismatic joint, fixed links without offset) -- the DEFAULT program bit for bit, populations 16 ... 200; ROBOT_FUZZ_BALANCE=1: links with mass and a BalanceGoal (whose sum over the links the device takes in walk order: agreement to rounding, DESIGN.md section 7 -- the strict comparison of this tool then reports it).  (Floating / planar joints are not drawn
here: tests/random_robot_cases.py draws them with a sampler of their own, on the device and in the host simulator.)  The trees and goal lists come from
tools/robot_gen.py.
ROBOT_FUZZ_HUGE=1: the ORACLE's solve of every robot alone, to find solves whose line search meets a candidate with a gene of magnitude in [2^32, 1e300)
(orc.huge_candidates: finite, but past the int32 quadrant of the sincos as first written, and below the candidate bound of that time); prints those cases and their count.
usage: python tools/robot_fuzz_hostsim.py [cases] [seed]   (seconds per case; exit code 1 on a mismatch)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "hostsim"), "-s"], check=True)
import parity_cases as pc  # noqa: E402
import robot_gen  # noqa: E402
from bio_ik_amd import ProblemTemplate, abi, solver  # noqa: E402
from oracle import orc  # noqa: E402


def huge_candidates_met(o, t, pop, steps, mode, fk, case):
    """the oracle's side of whole_solve alone: how many line-search candidates of magnitude [2^32, 1e300) it met"""
    from bio_ik_amd.workload import make_queries
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, 2, seed=case)
    p = abi.default_solve_params(population=pop, max_steps=steps, random_seed=11, mode=mode, fk_mode=fk, islands=1 + case % 2)
    before = orc.huge_candidates()
    o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=4)
    return orc.huge_candidates() - before


def whole_solve(h, o, t, pop, steps, mode, fk, case):
    """parity_cases.trajectory with NaNs compared as equal: a goal that is met exactly makes the quadratic line search divide 0 by 0 (ik_evolution_2.cpp:498-539),
    in the reference as here, and the NaN genes that follow must then be the same ones on both sides"""
    from bio_ik_amd.workload import make_queries
    seeds, params, _ = make_queries(t, o.active_variables, o.fk_genes, 2, seed=case)
    p = abi.default_solve_params(population=pop, max_steps=steps, random_seed=11, mode=mode, fk_mode=fk, islands=1 + case % 2)
    # (Until round 5 a solve in which an infinite step of the line search had put a joint WITHOUT limits at +-DBL_MAX was set aside here when the two sides parted:
    # 2 of 8000.  Round 6: such a candidate is no candidate on either side (quirk Q7, BIOIK_CANDIDATE_BOUND), and the two expressions that parted behind it are
    # known -- acos of a NaN (now tf2Acos's on both sides) and the struck-out zero terms of axis-aligned joints at sin / cos = inf.  Every solve is compared.)
    sa = o.solve_batch(p, orc.RNG_COUNTER, seeds, params, n_threads=4)
    sb = h.solve_batch(p, seeds, params)
    for a, b in zip(sa, sb):
        assert np.array_equal(a, b, equal_nan=True), "whole solves differ: %g" % np.nanmax(np.abs(np.asarray(a, float) - np.asarray(b, float)))
    return "  [NaN genes, the same on both sides]" if np.isnan(sa[0]).any() else ""


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    lib = solver.load_library(os.path.join(ROOT, "tests", "hostsim", "libbioik_hostsim.so"))
    orc.set_trig_mode(1)
    bad = skipped = met_huge = 0
    for case in range(n_cases):
        drawn = robot_gen.fuzz_case(rng, case, big=bool(os.environ.get("ROBOT_FUZZ_BIG")), plain=bool(os.environ.get("ROBOT_FUZZ_PLAIN")),
                                    balance=bool(os.environ.get("ROBOT_FUZZ_BALANCE")), gradient=bool(os.environ.get("ROBOT_FUZZ_GRADIENT")))
        if drawn is None:
            continue
        model, joints, tips, goals, fixed, desc, mode, fk, pop, steps = drawn
        try:
            t = ProblemTemplate(model, "g", goals, fixed_joints=fixed)
            try:
                o = orc.Oracle(t)
            except orc.OracleError as e:  # (what the reference refuses -- a goal on the variable of a mimic joint -- the device must refuse too)
                try:
                    solver.HipSolver(t, lib=lib)
                    bad += 1
                    print("%-3d BAD  %s: the oracle refuses (%s), the device does not" % (case, desc, e), flush=True)
                except solver.BioIKError as e2:
                    skipped += 1
                    print("%-3d skip %s (both refuse: %s | %s)" % (case, desc, e, e2), flush=True)
                continue
            if o.D == 0:
                skipped += 1
                print("%-3d skip %s (no active variable)" % (case, desc), flush=True)
                continue
            if os.environ.get("ROBOT_FUZZ_HUGE"):
                k = huge_candidates_met(o, t, pop, steps, mode, fk, case)
                if k:
                    met_huge += 1
                    print("%-3d HUGE %s: %d candidates with a gene of magnitude in [2^32, 1e300) (mode %s, fk %d, population %d, steps %d)" % (case, desc, k, mode, fk, pop, steps), flush=True)
                continue
            if os.environ.get("ROBOT_FUZZ_PLAIN"):  # the default program itself, bit for bit, populations up to the lane counts of the kernels compiled for one mapping
                os.environ["BIOIK_COMPILE_EXACT"] = "0"
                h = solver.HipSolver(t, lib=lib)
                pc.function_level(h, o, model, np.random.default_rng(case), n=16, exact_bits=True)
                nan_note = whole_solve(h, o, t, int(rng.choice([16, 64, 128, 200])), steps, mode, fk, case)
                print("%-3d ok   %s%s" % (case, desc, nan_note), flush=True)
                continue
            os.environ["BIOIK_COMPILE_EXACT"] = "1"
            h = solver.HipSolver(t, lib=lib)
            pc.function_level(h, o, model, np.random.default_rng(case), n=16, exact_bits=True)
            nan_note = whole_solve(h, o, t, pop, steps, mode, fk, case)
            os.environ["BIOIK_COMPILE_EXACT"] = "0"
            h2 = solver.HipSolver(t, lib=lib)
            pc.function_level(h2, o, model, np.random.default_rng(case), n=16, frame_tol=1e-12, fit_rtol=1e-9)
            print("%-3d ok   %s%s" % (case, desc, nan_note), flush=True)
        except solver.BioIKError as e:
            skipped += 1
            print("%-3d skip %s (%s)" % (case, desc, e), flush=True)
        except AssertionError as e:
            import traceback
            bad += 1
            print("%-3d BAD  [EXACT=%s] %s: %s @ %s" % (case, os.environ["BIOIK_COMPILE_EXACT"], desc, e, traceback.format_exc().splitlines()[-3].strip()), flush=True)
    if os.environ.get("ROBOT_FUZZ_HUGE"):
        print("%d cases, %d skipped, %d solves met a line-search candidate of magnitude in [2^32, 1e300); %d candidates at or beyond the bound of %g" % (
            n_cases, skipped, met_huge, orc.unbounded_candidates(), orc.candidate_bound()))
        sys.exit(0)
    print("%d cases, %d skipped (unsupported by the device, or no active variable), %d mismatches" % (n_cases, skipped, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
