"""sincos_small_cases.py on the device: the same cases as tests/test_hostsim_sincos_small.py through libbioik_hip.so, where the vote is one ballot per wavefront
-- bit for bit against bioik_sincos and the oracle, and device against host simulator."""
import numpy as np
import pytest

import sincos_small_cases as sc
from bio_ik_amd import solver
from bio_ik_amd.solver import HipSolver, device_count
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


def test_sincos_small_is_sincos_inside_the_bound(hostsim_lib):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    bound = sc.check_bound(None)
    assert bound == solver.sincos_small_bound(hostsim_lib)
    sc.check_small_is_sincos(solver.eval_arith, bound)
    x = sc.small_arguments(bound)
    assert np.array_equal(sc.bits(solver.eval_arith(sc.OP_SMALL, x)), sc.bits(solver.eval_arith(sc.OP_SMALL, x, lib=hostsim_lib)))


def test_voted_sincos_is_sincos(hostsim_lib):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    bound = sc.check_bound(None)
    dev = sc.check_vote(solver.eval_arith, bound)
    sim = sc.check_vote(lambda op, x: solver.eval_arith(op, x, lib=hostsim_lib), bound)
    for (x, a), (_, b) in zip(dev, sim):
        nan = np.isnan(x)
        assert np.all(np.isnan(a[nan])) and np.all(np.isnan(b[nan]))
        assert np.array_equal(sc.bits(a[~nan]), sc.bits(b[~nan]))


@pytest.mark.parametrize("kind", sc.GENE_SETS)
@pytest.mark.parametrize("name", sc.ROBOTS)
def test_function_level_walks(hostsim_lib, name, kind):
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    dev = sc.check_walk(name, kind, lambda t: HipSolver(t, device=0))
    sim = sc.check_walk(name, kind, lambda t: HipSolver(t, lib=hostsim_lib))
    assert all(np.array_equal(sc.bits(a), sc.bits(b)) for a, b in zip(dev, sim))
