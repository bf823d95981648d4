"""TouchGoal (tests/touch_cases.py) on a real MI355X: HipSolver(device=0) against the long-double restatement of the goal, and bit for bit against the host
simulator of the same kernel bodies (tests/hostsim/libbioik_hostsim.so) run in the same test.  Run with -s for the worst error / bound ratios."""
import numpy as np
import pytest

import random_robot_cases as rr
import touch_cases as tc
from bio_ik_amd import abi

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
    print("\n[touch, MI355X] " + s.line())


def hbm_arrays(a):
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(a).to(dev)

    def fetch():
        torch.cuda.synchronize(dev)
        return t.cpu().numpy()
    return t.data_ptr(), fetch


@pytest.mark.parametrize("name", sorted(tc.function_cases()))
def test_function_level(make_solver, stats, name):
    tc.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    tc.streamed(make_solver, hbm_arrays)


def test_refusals(make_solver):
    from bio_ik_amd.solver import load_library
    tc.refusals(make_solver, load_library())


@pytest.mark.parametrize("variant", ["primary", "secondary", "gd", "ranked"])
def test_whole_solve_and_simulator(make_solver, hostsim_lib, variant):
    """16 reachable queries, 64 steps, four islands, dtwist 1e-5: the asserts of touch_cases.verify_solve (measured: primary 16 of 16 solved, secondary 13 of
    16, gd 16 of 16, ranked 16 of 16 in row 0 and in row 1; the floor is 8), and results and steps bit for bit those of the host simulator."""
    from bio_ik_amd.solver import HipSolver
    h, t, seeds, params, p, res = tc.whole_solve(make_solver, variant)
    sim = HipSolver(t, lib=hostsim_lib)
    want = sim.solve_batch_ranked(p, seeds, params, 2, 0.0) if variant == "ranked" else sim.solve_batch(p, seeds, params)
    assert all(np.array_equal(a, b) for a, b in zip(res, want)), variant
    sim.close()
    h.close()


def test_mapping_independence(make_solver, monkeypatch):
    tc.mapping_independence(make_solver, monkeypatch)
