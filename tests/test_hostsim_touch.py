"""TouchGoal (tests/touch_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product stepped on the CPU against the long-double
restatement of the goal.  Run with -s for the worst error / bound ratios."""
import pytest

import random_robot_cases as rr
import touch_cases as tc
from bio_ik_amd.solver import HipSolver


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[touch, hostsim] " + s.line())


@pytest.mark.parametrize("name", sorted(tc.function_cases()))
def test_function_level(make_solver, stats, name):
    tc.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    tc.streamed(make_solver, lambda a: (a.ctypes.data, (lambda: a)))


def test_refusals(make_solver, hostsim_lib):
    tc.refusals(make_solver, hostsim_lib)


@pytest.mark.parametrize("variant", ["primary", "secondary", "gd", "ranked"])
def test_whole_solve(make_solver, variant):
    """16 reachable queries, 64 steps, four islands, dtwist 1e-5.  Measured on the host simulator (= the device, bit for bit): primary 16 of 16 solved, secondary
    13 of 16, gd 16 of 16, ranked 16 of 16 in row 0 and in row 1; the floor of the test is 8."""
    tc.whole_solve(make_solver, variant)[0].close()


def test_mapping_independence(make_solver, monkeypatch):
    # (the simulator steps every lane on one CPU thread: two queries and two steps here; tests/test_gpu_touch.py runs the whole-solve case)
    tc.mapping_independence(make_solver, monkeypatch, variants=("primary",), steps=2, n=2, islands=2)
