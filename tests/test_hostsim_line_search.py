"""line_search_cases.py on the host simulator: whole solves on the dense kernel through every path of its memetic line search, bit for bit against the
oracle -- and the count, from the oracle's own run, of the situations those solves are there for."""
import pytest

import limit_cases as lc
import line_search_cases as ls
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


@pytest.mark.parametrize("mode", sorted(ls.MODES))
@pytest.mark.parametrize("name", sorted(ls.CASES))
def test_line_search(hostsim_lib, report, name, mode):
    ls.solve(name, mode, lambda t: HipSolver(t, lib=hostsim_lib), report)


@pytest.mark.parametrize("mode", sorted(ls.MODES))
def test_the_situations_are_met(mode):
    """what the oracle's own run of the cases shows, counted on its first step (line_search_cases.situations) and by its own counter of candidates
    without bound: every situation the cases are there for, at least as often as EXPECTED_TOTAL says"""
    total = {}
    for name in sorted(ls.CASES):
        t, o, seeds, params, _ = ls.reference(name, mode)
        c = ls.situations(t, o, seeds, params, mode)
        assert c["searches"] == 2 * ls.QUERIES
        if name not in ("flat", "unbounded"):
            assert c["accepted"] >= ls.QUERIES // 3 and c["rejected"] + c["nan"] >= ls.QUERIES // 3, (name, c)  # (each case searches, and stops)
        for k, v in c.items():
            total[k] = total.get(k, 0) + int(v)
    for k, least in ls.EXPECTED_TOTAL[mode].items():
        assert total[k] >= least, (mode, k, total)
    # the step that is not a number (three equal support values), and the step without bound on a joint without limits
    t, o, seeds, params, _ = ls.reference("flat", mode)
    assert ls.situations(t, o, seeds, params, mode)["nan"] == 2 * ls.QUERIES
    assert ls.UNBOUNDED_MET[("unbounded", mode)] >= 2, ls.UNBOUNDED_MET
    # the second op of a lane (ops 32 and up) is a gene in one case
    assert ls.CASES["d31_fixed"][1][0] > 32 > ls.CASES["d31_fixed"][1][1]
