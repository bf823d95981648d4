"""ClearanceGoal (tests/clearance_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product stepped on the CPU against the long-double
restatement of the goal.  Run with -s for the worst error / bound ratios."""
import pytest

import clearance_cases as cc
import random_robot_cases as rr
from bio_ik_amd.solver import HipSolver


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[clearance, hostsim] " + s.line())


@pytest.mark.parametrize("name", sorted(cc.function_cases()))
def test_function_level(make_solver, stats, name):
    cc.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    cc.streamed(make_solver, lambda a: (a.ctypes.data, (lambda: a)))


def test_table_updates(make_solver, stats, hostsim_lib):
    cc.table_updates(make_solver, stats, hostsim_lib)


def test_refusals(make_solver, hostsim_lib):
    cc.refusals(make_solver, hostsim_lib)


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_whole_solve(make_solver, variant):
    """16 queries behind the column, 64 steps, four islands, dtwist 1e-5: every row flagged a success is clear of the column by the margin, recomputed in long
    double (clearance_cases.verify_solve).  "primary" also solves the same queries without the ClearanceGoals (clearance_cases.steering).  Found on the host
    simulator (= the device, bit for bit): without the goals 5 of the 16 answers are more than 1 cm inside the column (16 flagged a success: the PositionGoal alone);
    with them 16 of 16 succeed, the four deepest of those five among them, and no answer touches the column.  primary, secondary, ranked (row 0) and bounded: 16 of 16
    succeed; gd: 0 of 16 within 64 steps (its condition 1 is then empty; the fitness of every row is still checked).  No rate is asserted."""
    cc.whole_solve(make_solver, variant)[0].close()
    if variant == "primary":
        print("\n[clearance, hostsim] steering: %s" % cc.STEERING)


def test_mapping_independence(make_solver, monkeypatch):
    # (the simulator steps every lane on one CPU thread: two queries and two steps here; tests/test_gpu_clearance.py runs the whole-solve case)
    cc.mapping_independence(make_solver, monkeypatch, variants=("primary",), steps=2, n=2, islands=2)
