"""line_search_cases.py on the device: the same cases as tests/test_hostsim_line_search.py through libbioik_hip.so -- bit for bit against the oracle, and
device against host simulator."""
import numpy as np
import pytest

import limit_cases as lc
import line_search_cases as ls
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


@pytest.mark.parametrize("mode", sorted(ls.MODES))
@pytest.mark.parametrize("name", sorted(ls.CASES))
def test_line_search(hostsim_lib, report, name, mode):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    dev = ls.solve(name, mode, lambda t: HipSolver(t, device=0), report)
    sim = ls.solve(name, mode, lambda t: HipSolver(t, lib=hostsim_lib), report)
    assert all(np.array_equal(a, b) for a, b in zip(dev, sim))
