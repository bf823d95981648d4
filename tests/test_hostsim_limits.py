"""The limit cases of tests/limit_cases.py on the host simulator (tests/hostsim), which enforces the device's LDS rules: a launch of more than 64 KiB of
dynamic LDS fails unless its kernel was allowed that much, and nothing beyond a CU's 160 KiB launches -- both as BIOIK_ERR_HIP, as on the device."""
import numpy as np
import pytest

import limit_cases as lc
from bio_ik_amd.solver import HipSolver
from oracle import orc


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture
def report(monkeypatch, capfd):
    return lc.Report(monkeypatch, capfd)


@pytest.fixture(scope="module")
def sims(hostsim_lib, templates):
    return {k: HipSolver(t, lib=hostsim_lib) for k, t in templates.items()}


def host_arrays(a):
    """device pointers of the host simulator are host pointers"""
    return a.ctypes.data, (lambda: a)


def test_d63(make_solver, report):
    lc.d63(make_solver, report)


def test_64_ops_63_genes(make_solver, report):
    lc.ops64(make_solver, report)


def test_d32_d33(make_solver, report, monkeypatch):
    lc.d32_33(make_solver, report, monkeypatch)


def test_64_tips(make_solver, report):
    lc.t64(make_solver, report)


def test_24_plus_24_goals_and_4_balance_goals(make_solver):
    lc.goals_24_24(make_solver)


@pytest.mark.parametrize("cfg,pop", [(c, p) for c in ("c2", "c3", "c4") for p in lc.POPULATIONS if not (p == 1 and c != "c2")])
def test_population_thresholds(sims, oracles, templates, report, cfg, pop):
    """(population 1 only on C2: C3 and C4 have a secondary goal)"""
    lc.population_threshold(sims[cfg], oracles[cfg], templates[cfg], cfg, pop, report)


def test_small_linear_and_point_kernels(sims, oracles, templates, report):
    lc.small_linear_kernel(sims["c2"], oracles["c2"], templates["c2"], report)
    lc.point_kernel(sims["c2"], oracles["c2"], templates["c2"], report)


@pytest.mark.parametrize("which", ["under_64k", "over_64k", "beyond_160k"])
def test_lds_envelope(make_solver, which):
    name, model, t, b = [x for x in lc.envelope_problems() if x[0] == which][0]
    lc.envelope(make_solver, name, model, t, b, host_arrays)


@pytest.mark.parametrize("pop", [64, 256, 600])
def test_streamed_fitness_on_c4(sims, oracles, templates, pop):
    """C4 (31 ops): 73.5 KB of LDS at 256 lanes -- above 64 KiB, allowed explicitly"""
    lc.stream_fitness(sims["c4"], oracles["c4"], templates["c4"], pop, host_arrays)
