"""The random-robot cases of tests/random_robot_cases.py on a real MI355X (libbioik_hip.so, HipSolver(device=0)): 10^4 configurations per robot at function
level, whole solves over every solve kernel, the result contract with and without islands.  Prints the coverage, the worst error / bound ratios and the number
of success decisions that fell inside the error band."""
import numpy as np
import pytest

import limit_cases as lc
import random_robot_cases as rc
from oracle import orc
from tools import robot_gen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture(scope="module")
def make_solver():
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return lambda t: HipSolver(t, device=0)


def test_generator_coverage():
    cov = robot_gen.coverage(rc.cases())
    print("coverage:", cov)
    assert cov["joint_types"] == {0, 1, 2, 3, 4} and cov["continuous"] > 0
    assert cov["opcodes"] == set(range(17))
    assert cov["mimic_depth"] >= 2 and cov["tips_on_fixed_links"] > 0 and cov["fixed_joints"] > 0 and cov["secondary_goals"] > 0
    assert cov["not_walk_order"] > 0 and cov["refused"] > 0


def test_function_level_against_long_double(make_solver):
    stats = rc.Stats()
    for case in rc.cases(rc.SEEDS[::2]):
        rc.function_levels(case, make_solver, 10000, stats, n_edge=16)
    print(stats.line())
    assert stats.band > 0


def test_whole_solves_bit_for_bit(make_solver, monkeypatch, capfd):
    report = lc.Report(monkeypatch, capfd)
    ran, ran_multi = set(), set()
    for k, case in enumerate(rc.cases(rc.SEEDS[:24]) + rc.cases(rc.SEEDS[:24], multi=0.0, balance=False, walk=True)):
        got = rc.whole_solves(case, make_solver, report, monkeypatch, 2 * k)
        ran |= got
        if case.multi():
            ran_multi |= got
    for k, case in enumerate(rc.cases(rc.SEEDS[:12], walk=True, serial=True, plain=True)):  # (the default program: plain trees fold exactly)
        ran |= rc.whole_solves(case, make_solver, report, monkeypatch, k, rc.SERIAL_PLANS, exact=False)
    for k, case in enumerate(rc.cases(rc.SEEDS[:6], multi=0.0, balance=False, walk=True, plain=True)):
        ran |= rc.whole_solves(case, make_solver, report, monkeypatch, 3 * k, exact=False)
    with capfd.disabled():
        print("\nkernels:", sorted(ran), "| with floating / planar joints:", sorted(ran_multi))
    assert set(rc.KERNELS) <= ran, sorted(set(rc.KERNELS) - ran)
    assert "k_solve" in ran_multi


def test_huge_joint_angles(make_solver):
    """(d) of random_robot_cases: joint angles from 1e5 rad to the end of the shared sincos's domain"""
    stats = rc.Stats()
    for case in rc.huge_angle_cases():
        rc.huge_angle_levels(case, make_solver, stats)
    print(stats.line())
    assert stats.rows == 4 * 2 * 2 * rc.HUGE_ROWS


@pytest.mark.parametrize("islands,sync", [(1, 0), (3, 1)])
def test_result_contract(make_solver, islands, sync):
    stats = rc.Stats()
    solved = kept = with_sec = 0
    with rc.program(False):
        for case in rc.cases(rc.CONTRACT_SEEDS, gene_goals_secondary=True):
            made = rc.make_or_refuse(case, make_solver)
            if made is None:
                continue
            a, b, c = rc.result_contract(case, made[0], 100, np.random.default_rng(case.seed), stats, islands=islands, island_sync=sync)
            solved, kept, with_sec = solved + a, kept + b, with_sec + c
    print("solved %d (%d with secondary goals), kept at the seed %d |" % (solved, with_sec, kept), stats.line())
    assert with_sec > 0
