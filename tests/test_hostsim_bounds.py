"""Per-query variable bounds (tests/bounds_cases.py) on the host simulator (tests/hostsim): the bounded flavour of the product's kernel bodies, the staging of
a query's table of bounds and the launcher's gating stepped on the CPU, against the oracle on narrowed models bit for bit.  Every test ends with no write out
of bounds of a device block and nothing inside a capture that HIP would refuse."""
import pytest

import bounds_cases as bc
import limit_cases as lc
import migration_cases as mg
from bio_ik_amd.solver import HipSolver
from oracle import orc
from test_hostsim_sequences import HostDevice, counters


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def ctx(hostsim_lib, monkeypatch, capfd):
    count = counters(hostsim_lib)
    before = count()
    make = lambda t: HipSolver(t, lib=hostsim_lib)  # noqa: E731
    yield mg.Ctx(make, make, HostDevice(hostsim_lib), monkeypatch, lc.Report(monkeypatch, capfd))
    assert count() == before, "a write out of bounds of a device block, or something HIP refuses inside a capture (see the [hostsim] lines on stderr)"


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


def test_plugin_consistency_limits(ctx, pr2, hostsim_shim):
    bc.b6_plugin(ctx, pr2, hostsim_shim)
