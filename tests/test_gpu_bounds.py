"""Per-query variable bounds (tests/bounds_cases.py) on a real MI355X: k_solve_bounded and k_solve_point_bounded against the oracle on narrowed models and
against the host simulator of the same kernel bodies, bit for bit; the entry points' identities, a capture with two replays, the refusals."""
import pytest

import bounds_cases as bc
import limit_cases as lc
import migration_cases as mg
from oracle import orc
from test_gpu_sequences import TorchDevice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def ctx(hostsim_lib, monkeypatch, capfd):
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mg.Ctx(lambda t: HipSolver(t, device=0), lambda t: HipSolver(t, lib=hostsim_lib), TorchDevice(), monkeypatch, lc.Report(monkeypatch, capfd))


@pytest.mark.parametrize("name", ["arm", "mimic", "gnarly", "jv"])
def test_rule_against_its_restatement(ctx, pr2, name):
    bc.b1_rule(ctx, pr2, name)


@pytest.mark.parametrize("case", sorted(bc.SOLVES))
def test_solved_as_if_the_model_had_these_bounds(ctx, pr2, case):
    bc.b2_as_if(ctx, pr2, case)


def test_the_windows_do_what_the_oracle_did_with_them(ctx, pr2):
    bc.b2_table_is_what_the_issue_measured(ctx, pr2)


def test_no_bounds_is_the_plain_call(ctx, pr2):
    bc.b3_no_bounds_is_the_plain_call(ctx, pr2)


def test_host_submit_and_device_forms_agree_and_shards_too(ctx, pr2):
    bc.b3_three_forms(ctx, pr2)


def test_migration_handovers_and_the_throughput_schedule(ctx, pr2):
    bc.b3_plans(ctx, pr2)


def test_capture_and_two_replays(ctx, pr2):
    bc.b3_capture(ctx, pr2)


def test_seeds_inside_give_solutions_inside(ctx, pr2):
    bc.b4_inside(ctx, pr2)


def test_one_null_array_is_refused(ctx, pr2):
    bc.b5_one_null(ctx, pr2)


def test_refused_where_the_table_no_longer_fits_a_cu(ctx, pr2):
    bc.b5_lds_edge(ctx, pr2)


def test_plugin_consistency_limits(ctx, pr2):
    bc.b6_plugin(ctx, pr2, None)
