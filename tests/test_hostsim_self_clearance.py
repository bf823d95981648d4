"""SelfClearanceGoal (tests/self_clearance_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product stepped on the CPU against the
long-double restatement of the goal.  Run with -s for the worst error / bound ratios."""
import pytest

import random_robot_cases as rr
import self_clearance_cases as sc
from bio_ik_amd.solver import HipSolver


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[self clearance, hostsim] " + s.line())


@pytest.mark.parametrize("name", sorted(sc.function_cases()))
def test_function_level(make_solver, stats, name):
    sc.function_level(make_solver, name, stats, n=200)


def test_symmetry(make_solver, stats):
    sc.symmetry(make_solver, stats)


def test_streamed_fitness(make_solver):
    sc.streamed(make_solver, lambda a: (a.ctypes.data, (lambda: a)))


def test_refusals(make_solver, hostsim_lib):
    sc.refusals(make_solver, hostsim_lib)


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_whole_solve(make_solver, variant):
    """PR2-like `all`, 16 queries whose wrist targets make the arms cross, 64 steps, four islands, dtwist 1e-5, three spheres along each forearm: every row flagged a
    success has no pair of forearm spheres deeper than dtwist / weight inside the margin, recomputed in long double (self_clearance_cases.verify_solve).  "primary"
    also solves the same queries without the SelfClearanceGoal (self_clearance_cases.steering); the two counts it asserts are those found on the host simulator
    (= the device, bit for bit), stated at self_clearance_cases.WITHOUT_PENETRATING / WITH_SUCCESS."""
    sc.whole_solve(make_solver, variant)[0].close()
    if variant == "primary":
        print("\n[self clearance, hostsim] steering: %s" % sc.STEERING)


def test_mapping_independence(make_solver, monkeypatch):
    # (the simulator steps every lane on one CPU thread: two queries, two steps and 32 individuals here; tests/test_gpu_self_clearance.py runs the whole-solve case)
    sc.mapping_independence(make_solver, monkeypatch, steps=2, n=2, islands=2, population=32)
