"""TouchGoal on cylinders and cones (tests/touch_disk_cases.py) on a real MI355X: HipSolver(device=0) against the long-double restatement of the goal, and bit
for bit against the host simulator of the same kernel bodies (tests/hostsim/libbioik_hostsim.so) run in the same test.  Run with -s for every case's worst
error and the worst error / bound ratios."""
import numpy as np
import pytest

import random_robot_cases as rr
import touch_disk_cases as td
from test_gpu_touch import hbm_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture
def make_solver():
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return lambda t: HipSolver(t, device=0)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[touch disks, MI355X] " + s.line())


@pytest.mark.parametrize("name", sorted(td.function_cases()))
def test_function_level(make_solver, stats, name):
    td.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    td.streamed(make_solver, hbm_arrays)


def test_refusals(make_solver):
    from bio_ik_amd.solver import load_library
    td.refusals(make_solver, load_library())


@pytest.mark.parametrize("variant", ["primary", "secondary", "gd", "ranked"])
def test_whole_solve_and_simulator(make_solver, hostsim_lib, variant):
    """16 reachable queries on a cylinder, 64 steps, four islands, dtwist 1e-5: the asserts of touch_disk_cases.verify_solve (the floor is 8 solved), and
    results and steps bit for bit those of the host simulator."""
    from bio_ik_amd.solver import HipSolver
    h, t, seeds, params, p, res = td.whole_solve(make_solver, variant)
    sim = HipSolver(t, lib=hostsim_lib)
    want = sim.solve_batch_ranked(p, seeds, params, 2, 0.0) if variant == "ranked" else sim.solve_batch(p, seeds, params)
    assert all(np.array_equal(a, b) for a, b in zip(res, want)), variant
    sim.close()
    h.close()


def test_mapping_independence(make_solver, monkeypatch):
    td.mapping_independence(make_solver, monkeypatch)
