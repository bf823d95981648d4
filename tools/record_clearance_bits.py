"""Records the fitness bits of three sphere-only clearance cases into tests/golden/clearance_parent_bits.npz.

Run ONCE, on the commit in front of the one that gave links capsules, on the host simulator (tests/hostsim):

    python tools/record_clearance_bits.py

The capsule change promises that a model without capsules gives exactly the bits it gave before, for opcode 19 and for opcode 20; the tests of
tests/capsule_cases.py (unchanged_bits) recompute `bits()` on the simulator and on the device and compare with numpy.array_equal.  The cases are existing ones,
taken as they stand: clearance_cases "points_3_obstacles_9", self_clearance_cases "points_3_other_9" and "beside_world_clearance".  Per case the primary fitness of
200 random individuals under exact FK and of 25 linearised phenotypes around the one of them with the largest fitness."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clearance_parent_bits.npz")
CASES = (("clearance_cases", "points_3_obstacles_9"), ("self_clearance_cases", "points_3_other_9"), ("self_clearance_cases", "beside_world_clearance"))


def bits(make_solver, n=200):
    """{"<case>/exact": (n,), "<case>/linear": (25,)} on the library behind make_solver(template)"""
    for d in (ROOT, os.path.join(ROOT, "tests")):
        if d not in sys.path:
            sys.path.insert(0, d)
    import importlib

    import clearance_cases as cc
    import np_goals
    from bio_ik_amd import ProblemTemplate, abi
    out = {}
    for module, name in CASES:
        model, group, goals = importlib.import_module(module).function_cases()[name]
        t = ProblemTemplate(model, group, goals)
        h = make_solver(t)
        pr = np_goals.Problem(t, h.active_variables, h.tip_links)
        rng = np.random.default_rng(sum(map(ord, name)))
        seed, genes = cc.population(model, pr, rng, n)
        params = t.pack_params()
        out[name + "/exact"] = h.fitness(abi.FK_EXACT, seed, params, genes)[0]
        base = genes[int(np.argmax(out[name + "/exact"]))]  # (an individual that penetrates: its neighbours do too)
        near = np.ascontiguousarray(base + 0.02 * rng.normal(size=(25, len(pr.active))))
        out[name + "/linear"] = h.fitness(abi.FK_LINEAR, seed, params, near, base)[0]
        h.close()
    return out


def main():
    import subprocess
    sys.path.insert(0, ROOT)
    from bio_ik_amd import solver
    d = os.path.join(ROOT, "tests", "hostsim")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    lib = solver.load_library(os.path.join(d, "libbioik_hostsim.so"))
    out = bits(lambda t: solver.HipSolver(t, lib=lib))
    assert all(np.any(v > 0.0) for v in out.values())
    np.savez(GOLDEN, **out)
    print("wrote %s: %s" % (GOLDEN, {k: v.shape for k, v in out.items()}))


if __name__ == "__main__":
    main()
