"""The limit cases of tests/limit_cases.py on a real MI355X, through the C-ABI of libbioik_hip.so: every entry point at the declared size limits, the
mapping thresholds from both sides, the LDS envelope per entry point.  (The host-simulator suite, tests/test_hostsim_limits.py, runs the same cases
under the device's LDS rules first: nothing here depends on the runtime refusing a launch.)"""
import numpy as np
import pytest

import limit_cases as lc
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def make_solver():
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return lambda t: HipSolver(t, device=0)


@pytest.fixture
def report(monkeypatch, capfd):
    return lc.Report(monkeypatch, capfd)


@pytest.fixture(scope="module")
def gpus(templates):
    from bio_ik_amd.solver import HipSolver
    return {k: HipSolver(t, device=0) for k, t in templates.items()}


def hbm_arrays(a):
    """a copy of `a` in HBM (torch only supplies memory): its pointer, and a fetch that waits for the device and reads it back"""
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(a).to(dev)

    def fetch():
        torch.cuda.synchronize(dev)
        return t.cpu().numpy()
    return t.data_ptr(), fetch


def test_d63(make_solver, report):
    lc.d63(make_solver, report)


def test_64_ops_63_genes(make_solver, report):
    lc.ops64(make_solver, report)


def test_d32_d33(make_solver, report, monkeypatch):
    lc.d32_33(make_solver, report, monkeypatch)


def test_64_tips(make_solver, report):
    lc.t64(make_solver, report, steps=(1, 3))


def test_24_plus_24_goals_and_4_balance_goals(make_solver):
    lc.goals_24_24(make_solver)


@pytest.mark.parametrize("cfg,pop", [(c, p) for c in ("c2", "c3", "c4") for p in lc.POPULATIONS if not (p == 1 and c != "c2")])
def test_population_thresholds(gpus, oracles, templates, report, cfg, pop):
    lc.population_threshold(gpus[cfg], oracles[cfg], templates[cfg], cfg, pop, report)


def test_small_linear_and_point_kernels(gpus, oracles, templates, report):
    lc.small_linear_kernel(gpus["c2"], oracles["c2"], templates["c2"], report)
    lc.point_kernel(gpus["c2"], oracles["c2"], templates["c2"], report)


@pytest.mark.parametrize("which", ["under_64k", "over_64k", "beyond_160k"])
def test_lds_envelope(make_solver, which):
    name, model, t, b = [x for x in lc.envelope_problems() if x[0] == which][0]
    lc.envelope(make_solver, name, model, t, b, hbm_arrays)


@pytest.mark.parametrize("pop", [64, 256, 600])
def test_streamed_fitness_on_c4(gpus, oracles, templates, pop):
    """C4 (31 ops): 73.5 KB of LDS at 256 lanes -- above 64 KiB, allowed explicitly"""
    lc.stream_fitness(gpus["c4"], oracles["c4"], templates["c4"], pop, hbm_arrays, units=4)
