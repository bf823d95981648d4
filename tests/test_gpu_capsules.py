"""Capsules as link collision shapes (tests/capsule_cases.py) on a real MI355X: HipSolver(device=0) against the long-double restatement, and bit for bit against the
host simulator of the same kernel bodies (tests/hostsim/libbioik_hostsim.so) run in the same test.  Run with -s for the worst error / bound ratios."""
import numpy as np
import pytest

import base_link_cases as bl
import capsule_cases as cap
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
    print("\n[capsules, MI355X] " + s.line())


@pytest.mark.parametrize("name", sorted(cap.function_cases()))
def test_function_level(make_solver, make_sim, stats, name):
    """against the restatement, and every row of both FK modes bit for bit the host simulator's"""
    got = cap.function_level(make_solver, name, stats)
    want = cap.function_level(make_sim, name, rr.Stats())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


def test_symmetry(make_solver, stats):
    cap.symmetry(make_solver, stats)


def test_far_from_the_base_stays_finite(make_solver):
    cap.zero_quaternion(make_solver)


def test_touch_goal_reads_a_capsule_as_its_end_spheres(make_solver, make_sim):
    got, want = cap.touch_twins(make_solver), cap.touch_twins(make_sim)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_unchanged_bits_without_capsules(make_solver):
    cap.unchanged_bits(make_solver)


@pytest.mark.parametrize("variant", cap.VARIANTS)
def test_whole_solve_and_simulator(make_solver, make_sim, variant):
    """16 queries whose wrist targets make the arms cross, 64 steps, four islands, dtwist 1e-5, one capsule per forearm: the asserts of capsule_cases.verify_solve and,
    for "primary", of capsule_cases.steering (the counts found on the host simulator, asserted here as found) -- and results and steps bit for bit those of the host
    simulator."""
    h, t, seeds, params, p, res = cap.whole_solve(make_solver, variant)
    bounds = sc.solve_bounds(t, seeds)[1] if variant == "bounded" else None  # (whole_solve hands back the seeds it solved from)
    want = bl.sharded(lambda: make_sim(t), "ranked" if variant == "ranked" else "plain", p, seeds, params, bounds, 8)  # (the simulator in slices on 8 threads: sooner)
    assert all(np.array_equal(a, b) for a, b in zip(res, want)), variant
    h.close()


def test_arm_solve_and_simulator(make_solver, make_sim):
    h, t, seeds, params, p, res = cap.arm_solve(make_solver)
    want = bl.sharded(lambda: make_sim(t), "plain", p, seeds, params, None, 8)
    assert all(np.array_equal(a, b) for a, b in zip(res, want))
    h.close()


def test_mapping_independence(make_solver, monkeypatch):
    cap.mapping_independence(make_solver, monkeypatch)
