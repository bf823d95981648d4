"""SelfClearanceGoal (tests/self_clearance_cases.py) on a real MI355X: HipSolver(device=0) against the long-double restatement of the goal, and bit for bit against the
host simulator of the same kernel bodies (tests/hostsim/libbioik_hostsim.so) run in the same test.  Run with -s for the worst error / bound ratios."""
import numpy as np
import pytest

import base_link_cases as bl
import random_robot_cases as rr
import self_clearance_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture
def make_solver():
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return lambda t: HipSolver(t, device=0)


@pytest.fixture
def make_sim(hostsim_lib):
    from bio_ik_amd.solver import HipSolver
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[self clearance, MI355X] " + s.line())


def hbm_arrays(a):
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(a).to(dev)

    def fetch():
        torch.cuda.synchronize(dev)
        return t.cpu().numpy()
    return t.data_ptr(), fetch


@pytest.mark.parametrize("name", sorted(sc.function_cases()))
def test_function_level(make_solver, make_sim, stats, name):
    """against the restatement, and every row of both FK modes bit for bit the host simulator's"""
    got = sc.function_level(make_solver, name, stats, n=200)
    want = sc.function_level(make_sim, name, rr.Stats(), n=200)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


def test_symmetry(make_solver, stats):
    sc.symmetry(make_solver, stats)


def test_streamed_fitness(make_solver):
    sc.streamed(make_solver, hbm_arrays)


def test_refusals(make_solver):
    from bio_ik_amd.solver import load_library
    sc.refusals(make_solver, load_library())


@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_whole_solve_and_simulator(make_solver, make_sim, variant):
    """16 queries whose wrist targets make the arms cross, 64 steps, four islands, dtwist 1e-5: the asserts of self_clearance_cases.verify_solve and, for "primary", of
    self_clearance_cases.steering -- without the SelfClearanceGoal 10 of the 16 answers have forearms more than 1 cm inside one another, with it 16 of 16 succeed
    (found on the host simulator, asserted here as found) -- and results and steps bit for bit those of the host simulator."""
    h, t, seeds, params, p, res = sc.whole_solve(make_solver, variant)
    bounds = sc.solve_bounds(t, seeds)[1] if variant == "bounded" else None  # (whole_solve hands back the seeds it solved from)
    want = bl.sharded(lambda: make_sim(t), "ranked" if variant == "ranked" else "plain", p, seeds, params, bounds, 8)  # (the simulator in slices on 8 threads: sooner)
    assert all(np.array_equal(a, b) for a, b in zip(res, want)), variant
    h.close()


def test_mapping_independence(make_solver, monkeypatch):
    sc.mapping_independence(make_solver, monkeypatch)
