"""Island migration (tests/migration_cases.py) on a real MI355X: HipSolver(device=0) against the restated rule, against the host simulator of the same kernel
bodies bit for bit, twice and under forced mappings, and through the Python plugin."""
import pytest

import limit_cases as lc
import migration_cases as mg
from test_gpu_sequences import TorchDevice

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx(hostsim_lib, monkeypatch, capfd):
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mg.Ctx(lambda t: HipSolver(t, device=0), lambda t: HipSolver(t, lib=hostsim_lib), TorchDevice(), monkeypatch, lc.Report(monkeypatch, capfd))


@pytest.mark.parametrize("name,islands", [("arm", 3), ("arm", 65), ("mimic", 3), ("mimic", 65), ("jv", 3), ("jv", 65)])
def test_rule_against_its_restatement(ctx, pr2, name, islands):
    mg.m1_rule(ctx, pr2, name, islands)


def test_identities(ctx, pr2):
    mg.m2_identities(ctx, pr2)


@pytest.mark.parametrize("name", sorted(mg.SOLVES))
def test_whole_solves_against_the_simulator(ctx, pr2, name):
    mg.m3_against_simulator(ctx, pr2, name)


def test_ranked_against_the_simulator(ctx, pr2):
    mg.m3_ranked(ctx, pr2)


@pytest.mark.parametrize("name", ["arm_n1_i64_e2_sync", "arm_n1_i65_e3", "jv_n3_i3_e3"])
def test_determinism(ctx, pr2, name):
    mg.m4_determinism(ctx, pr2, name)


def test_it_does_something_and_keeps_the_result_contract(ctx, pr2):
    mg.m5_does_something(ctx, pr2)


def test_refusals(ctx, pr2):
    mg.m6_refusals(ctx, pr2)


def test_refused_on_a_capturing_stream(ctx, pr2):
    mg.m6_capture(ctx, pr2)


def test_plugin_key_reaches_the_solver(ctx, pr2):
    mg.m6_plugin_key(ctx, pr2, None)
