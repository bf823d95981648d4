"""Capsules as link collision shapes (tests/capsule_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product stepped on the CPU against the
long-double restatement.  Run with -s for the worst error / bound ratios."""
import pytest

import capsule_cases as cap
import random_robot_cases as rr
from bio_ik_amd.solver import HipSolver


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[capsules, hostsim] " + s.line())


@pytest.mark.parametrize("name", sorted(cap.function_cases()))
def test_function_level(make_solver, stats, name):
    cap.function_level(make_solver, name, stats)


def test_symmetry(make_solver, stats):
    cap.symmetry(make_solver, stats)


def test_far_from_the_base_stays_finite(make_solver):
    cap.zero_quaternion(make_solver)


def test_touch_goal_reads_a_capsule_as_its_end_spheres(make_solver):
    cap.touch_twins(make_solver)


def test_unchanged_bits_without_capsules(make_solver):
    cap.unchanged_bits(make_solver)


@pytest.mark.parametrize("variant", cap.VARIANTS)
def test_whole_solve(make_solver, variant):
    """PR2-like `all`, 16 queries whose wrist targets make the arms cross, 64 steps, four islands, dtwist 1e-5, one capsule along each forearm: every row flagged a
    success has its forearm capsules no deeper than dtwist / weight inside the margin, recomputed in long double (capsule_cases.verify_solve).  "primary" also solves
    the same queries without the SelfClearanceGoal (capsule_cases.steering); the two counts it asserts are those found on the host simulator."""
    cap.whole_solve(make_solver, variant)[0].close()
    if variant == "primary":
        print("\n[capsules, hostsim] steering: %s" % cap.STEERING)


def test_arm_solve(make_solver):
    """the right arm with a capsule on its forearm behind the column of nine spheres (opcode 19), the same two conditions"""
    cap.arm_solve(make_solver)[0].close()
    print("\n[capsules, hostsim] arm steering: %s" % cap.ARM_STEERING)


def test_mapping_independence(make_solver, monkeypatch):
    # (the simulator steps every lane on one CPU thread: two queries, two steps and 32 individuals here; tests/test_gpu_capsules.py runs the whole-solve case)
    cap.mapping_independence(make_solver, monkeypatch, steps=2, n=2, islands=2, population=32)
