"""sincos_small_cases.py on the host simulator: bioik_sincos_small, the walks' voted sincos (each lane answers the vote with its own predicate there) and
function-level walks on both sides of BIOIK_SINCOS_SMALL, bit for bit."""
import pytest

import sincos_small_cases as sc
from bio_ik_amd import solver
from bio_ik_amd.solver import HipSolver
from oracle import orc


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    """bit-exact comparisons need the oracle on the sincos it shares with the device (oracle/orc_model.h)"""
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


def test_the_bound_rounds_to_quadrant_zero(hostsim_lib):
    sc.check_bound(hostsim_lib)


def test_sincos_small_is_sincos_inside_the_bound(hostsim_lib):
    sc.check_small_is_sincos(lambda op, x: solver.eval_arith(op, x, lib=hostsim_lib), sc.check_bound(hostsim_lib))


def test_voted_sincos_is_sincos(hostsim_lib):
    sc.check_vote(lambda op, x: solver.eval_arith(op, x, lib=hostsim_lib), sc.check_bound(hostsim_lib))


@pytest.mark.parametrize("kind", sc.GENE_SETS)
@pytest.mark.parametrize("name", sc.ROBOTS)
def test_function_level_walks(hostsim_lib, name, kind):
    sc.check_walk(name, kind, lambda t: HipSolver(t, lib=hostsim_lib))
