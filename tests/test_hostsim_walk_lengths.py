"""walk_length_cases.py on the host simulator: the chain walk of the kernels compiled for one mapping (two joints per trip on a serial chain whose tips hang
behind its last op, one per trip for the last joints and otherwise) at every chain length and joint order at which it can go wrong, whole solves bit for bit against the oracle."""
import pytest

import limit_cases as lc
import walk_length_cases as wl
from bio_ik_amd.solver import HipSolver
from oracle import orc


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    """bit-exact comparisons need the oracle on the sincos it shares with the device (oracle/orc_model.h)"""
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def report(monkeypatch, capfd):
    return lc.Report(monkeypatch, capfd)


@pytest.mark.parametrize("schedule", sorted(wl.SCHEDULES))
@pytest.mark.parametrize("name", sorted(wl.CASES))
def test_walk_lengths(hostsim_lib, report, monkeypatch, name, schedule):
    wl.solve(name, schedule, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch)


def test_the_cases_are_what_they_say(hostsim_lib, report, monkeypatch, capfd):
    """the joint programs behind the names (BIOIK_SOLVE_REPORT prints them): the chain lengths, the right arm's prefix of one op, which cases have every
    tip behind the last op"""
    import re
    want = {"snake1": (1, 0), "snake2": (2, 0), "snake3": (3, 0), "snake4": (4, 0), "snake7": (7, 0), "snake8": (8, 0), "right_arm": (8, 1),
            "sliding_chain": (7, 0), "goal_behind_op2": (6, 0), "goal_behind_op3": (6, 0)}
    for name, (ops, prefix) in want.items():
        t = wl.reference(name)[0]
        report.read()
        h = HipSolver(t, lib=hostsim_lib)
        wl.solve(name, "throughput", lambda _t: h, report, monkeypatch)
        assert h.T == (1 if wl.CASES[name][1] else 2)
        report.read()
        assert lc.shape_of(h, t, report)[0] == ops, name
    assert sorted(want) == sorted(wl.CASES)
