"""Island migration (tests/migration_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product, migrate_mark and migrate_coop among them,
and the launcher's migration plan stepped on the CPU.  Every test ends with no write out of bounds of a device block and nothing inside a capture that HIP would
refuse."""
import pytest

import limit_cases as lc
import migration_cases as mg
from bio_ik_amd.solver import HipSolver
from test_hostsim_sequences import HostDevice, counters


@pytest.fixture
def ctx(hostsim_lib, monkeypatch, capfd):
    count = counters(hostsim_lib)
    before = count()
    make = lambda t: HipSolver(t, lib=hostsim_lib)  # noqa: E731
    yield mg.Ctx(make, make, HostDevice(hostsim_lib), monkeypatch, lc.Report(monkeypatch, capfd))
    assert count() == before, "a write out of bounds of a device block, or something HIP refuses inside a capture (see the [hostsim] lines on stderr)"


@pytest.mark.parametrize("name,islands", [("arm", 3), ("arm", 65), ("mimic", 3), ("mimic", 65), ("jv", 3), ("jv", 65)])
def test_rule_against_its_restatement(ctx, pr2, name, islands):
    mg.m1_rule(ctx, pr2, name, islands)


def test_identities(ctx, pr2):
    mg.m2_identities(ctx, pr2)


@pytest.mark.parametrize("name", sorted(mg.SOLVES))
def test_whole_solves(ctx, pr2, name):
    """(here the library under test IS the simulator: a fresh handle against the shared result, and the launches the plan promises)"""
    mg.m3_against_simulator(ctx, pr2, name)


def test_ranked(ctx, pr2):
    mg.m3_ranked(ctx, pr2)


def test_determinism(ctx, pr2):
    mg.m4_determinism(ctx, pr2, "arm_n3_i2_e2")
    mg.m4_determinism(ctx, pr2, "jv_n3_i3_e3")


def test_it_does_something_and_keeps_the_result_contract(ctx, pr2):
    mg.m5_does_something(ctx, pr2)


def test_refusals(ctx, pr2):
    mg.m6_refusals(ctx, pr2)


def test_refused_on_a_capturing_stream(ctx, pr2):
    mg.m6_capture(ctx, pr2)


def test_plugin_key_reaches_the_solver(ctx, pr2, hostsim_shim):
    mg.m6_plugin_key(ctx, pr2, hostsim_shim)
