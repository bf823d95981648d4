"""TouchGoal on cylinders and cones (tests/touch_disk_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product stepped on the CPU
against the long-double restatement of the goal.  Run with -s for every case's worst error and the worst error / bound ratios."""
import pytest

import random_robot_cases as rr
import touch_disk_cases as td
from bio_ik_amd.solver import HipSolver


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[touch disks, hostsim] " + s.line())


@pytest.mark.parametrize("name", sorted(td.function_cases()))
def test_function_level(make_solver, stats, name):
    td.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    td.streamed(make_solver, lambda a: (a.ctypes.data, (lambda: a)))


def test_refusals(make_solver, hostsim_lib):
    td.refusals(make_solver, hostsim_lib)


@pytest.mark.parametrize("variant", ["primary", "secondary", "gd", "ranked"])
def test_whole_solve(make_solver, variant):
    """16 reachable queries on a cylinder, 64 steps, four islands, dtwist 1e-5; the floor of the test is 8 solved (tests/test_gpu_touch_disks.py has the counts)."""
    td.whole_solve(make_solver, variant)[0].close()


def test_mapping_independence(make_solver, monkeypatch):
    # (the simulator steps every lane on one CPU thread: two queries and two steps here; tests/test_gpu_touch_disks.py runs 8 queries and 8 steps)
    td.mapping_independence(make_solver, monkeypatch, variants=("primary",), steps=2, n=2, islands=2)
