"""selection_cases.py on the device: the same cases as tests/test_hostsim_dense_selection.py through libbioik_hip.so -- bit for bit against the oracle (the
coarse-fitness cases: against the library's latency mapping), and device against host simulator."""
import numpy as np
import pytest

import limit_cases as lc
import selection_cases as sc
from bio_ik_amd.solver import HipSolver, device_count
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def report(monkeypatch, capfd):
    return lc.Report(monkeypatch, capfd)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_dense_selection(hostsim_lib, report, monkeypatch, name):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    dev = sc.solve(name, lambda t: HipSolver(t, device=0), report, monkeypatch)
    sim = sc.solve(name, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch)
    assert all(np.array_equal(a, b) for a, b in zip(dev, sim))


def test_coarse_values_make_ties(monkeypatch):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert sc.coarse_values_change_the_search(lambda t: HipSolver(t, device=0), monkeypatch)
