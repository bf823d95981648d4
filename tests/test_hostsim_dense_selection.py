"""selection_cases.py on the host simulator: whole solves on the dense kernel through every path of its selection by keys and its winners' copy, bit for
bit against the oracle -- and the count, from the oracle's own first steps, of the situations those solves are there for."""
import pytest

import limit_cases as lc
import selection_cases as sc
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


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_dense_selection(hostsim_lib, report, monkeypatch, name):
    sc.solve(name, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch)


def test_coarse_values_make_ties(hostsim_lib, monkeypatch):
    assert sc.coarse_values_change_the_search(lambda t: HipSolver(t, lib=hostsim_lib), monkeypatch)


def test_the_situations_are_met():
    """what the oracle's own first steps of the counted cases show (selection_cases.situations): every situation the cases are there for occurred -- a child
    took first place, a child took second place, both parents stayed, the keys put the selection in doubt (with 50 dropped bits in every generation,
    with the product's ten in none of these), several best children tied"""
    total, per_case = {}, {}
    for name in sc.COUNTED:
        c = per_case[name] = sc.situations(name)
        assert c["generations"] == 2 * 8 * sc.CASES[name]["n"]
        for k, v in c.items():
            total[k] = total.get(k, 0) + int(v)
    for k in ("child_first", "child_second", "parents_stay", "doubt", "ties"):
        assert total[k] >= 1, (k, total)
    # every chain and both forms of the keys see children win both places
    for name in ("pop128", "pop200", "d20_pop128", "d31_fixed_pop128"):
        assert per_case[name]["child_first"] >= 1 and per_case[name]["child_second"] >= 1, (name, per_case[name])
    # the widest keys: the exact path in most generations, for four and for eight keys per lane and for one winner per pass
    for name in ("drop50", "drop50_pop255", "drop50_d20"):
        assert 2 * per_case[name]["doubt"] > per_case[name]["generations"], (name, per_case[name])
    # queries that start at their goal: the parents stay in every generation of those queries' first step
    for name in ("at_goal", "at_goal_d20_pop160"):
        assert 2 * per_case[name]["parents_stay"] == per_case[name]["generations"] == 2 * per_case[name]["child_first"], (name, per_case[name])
    # joints without range: every generation ties and both parents stay
    c = per_case["no_range_pop128"]
    assert c["ties"] == c["parents_stay"] == c["generations"], c
