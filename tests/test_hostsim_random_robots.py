"""The random-robot cases of tests/random_robot_cases.py in the host simulator (tests/hostsim): fewer robots, configurations and queries than on the device
(tests/test_gpu_random_robots.py)."""
import numpy as np
import pytest

import limit_cases as lc
import random_robot_cases as rc
from bio_ik_amd.solver import HipSolver
from oracle import orc
from tools import robot_gen


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


def test_generator_coverage():
    cov = robot_gen.coverage(rc.cases())
    print("coverage:", cov)
    assert cov["joint_types"] == {0, 1, 2, 3, 4} and cov["continuous"] > 0
    assert cov["opcodes"] == set(range(17))
    assert cov["mimic_depth"] >= 2 and cov["tips_on_fixed_links"] > 0 and cov["fixed_joints"] > 0 and cov["secondary_goals"] > 0
    assert cov["not_walk_order"] > 0 and cov["refused"] > 0


def test_function_level_against_long_double(hostsim_lib):
    stats = rc.Stats()
    for case in rc.cases(rc.SEEDS[::3]):
        rc.function_levels(case, lambda t: HipSolver(t, lib=hostsim_lib), 200, stats, n_edge=4)
    print(stats.line())
    assert stats.band > 0


def test_whole_solves_bit_for_bit(hostsim_lib, monkeypatch, capfd):
    report = lc.Report(monkeypatch, capfd)
    ran, ran_multi = set(), set()
    for k, case in enumerate(rc.cases(rc.SEEDS[:12]) + rc.cases(rc.SEEDS[:24], multi=0.0, balance=False, walk=True)):
        got = rc.whole_solves(case, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch, 2 * k)
        ran |= got
        if case.multi():
            ran_multi |= got
    for k, case in enumerate(rc.cases(rc.SEEDS[:12], walk=True, serial=True, plain=True)):  # (the default program: plain trees fold exactly)
        ran |= rc.whole_solves(case, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch, k, rc.SERIAL_PLANS, exact=False)
    for k, case in enumerate(rc.cases(rc.SEEDS[:6], multi=0.0, balance=False, walk=True, plain=True)):
        ran |= rc.whole_solves(case, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch, 3 * k, exact=False)
    with capfd.disabled():
        print("\nkernels:", sorted(ran), "| with floating / planar joints:", sorted(ran_multi))
    assert set(rc.KERNELS) <= ran, sorted(set(rc.KERNELS) - ran)
    assert "k_solve" in ran_multi


def test_huge_joint_angles(hostsim_lib):
    """(d) of random_robot_cases: joint angles from 1e5 rad to the end of the shared sincos's domain"""
    stats = rc.Stats()
    for case in rc.huge_angle_cases():
        rc.huge_angle_levels(case, lambda t: HipSolver(t, lib=hostsim_lib), stats)
    print(stats.line())
    assert stats.rows == 4 * 2 * 2 * rc.HUGE_ROWS


@pytest.mark.parametrize("islands,sync", [(1, 0), (3, 1)])
def test_result_contract(hostsim_lib, islands, sync):
    stats = rc.Stats()
    solved = kept = with_sec = 0
    with rc.program(False):
        for case in rc.cases([8, 13, 26, 31, 39], gene_goals_secondary=True):
            made = rc.make_or_refuse(case, lambda t: HipSolver(t, lib=hostsim_lib))
            if made is None:
                continue
            a, b, c = rc.result_contract(case, made[0], 10, np.random.default_rng(case.seed), stats, islands=islands, island_sync=sync, steps=6)
            solved, kept, with_sec = solved + a, kept + b, with_sec + c
    print("solved %d (%d with secondary goals), kept at the seed %d |" % (solved, with_sec, kept), stats.line())
    assert with_sec > 0
