"""walk_length_cases.py on the device: the same cases as tests/test_hostsim_walk_lengths.py through libbioik_hip.so -- bit for bit against the oracle, and
device against host simulator."""
import numpy as np
import pytest

import limit_cases as lc
import walk_length_cases as wl
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


@pytest.mark.parametrize("schedule", sorted(wl.SCHEDULES))
@pytest.mark.parametrize("name", sorted(wl.CASES))
def test_walk_lengths(hostsim_lib, report, monkeypatch, name, schedule):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    dev = wl.solve(name, schedule, lambda t: HipSolver(t, device=0), report, monkeypatch)
    sim = wl.solve(name, schedule, lambda t: HipSolver(t, lib=hostsim_lib), report, monkeypatch)
    assert all(np.array_equal(a, b) for a, b in zip(dev, sim))
