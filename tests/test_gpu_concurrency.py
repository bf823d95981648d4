"""The concurrency cases of tests/concurrency_cases.py on a real MI355X, in ONE process with at most eight threads: nothing synchronises between the enqueues of a
round, so the overlap is the device's own.  K8 (graphs captured from two streams of one handle, replayed together; single-stream, linear graphs as in S4) and K9
(chip-filling calls together) exist here only.  Graphs are destroyed before their handle."""
import pytest

import concurrency_cases as cc
import limit_cases as lc
from bio_ik_amd import ProblemTemplate
from conftest import gnarly_goals
from oracle import orc
from test_gpu_sequences import TorchDevice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def seq(templates, oracles, monkeypatch, capfd):
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return cc.Concurrency(lambda t: HipSolver(t, device=0), TorchDevice(), lc.Report(monkeypatch, capfd), monkeypatch, templates, oracles)


@pytest.mark.parametrize("cfg", ["c2", "c4"])
def test_k1_streams_of_one_handle(seq, cfg):
    cc.k1_streams(seq, cfg)


@pytest.mark.parametrize("cfg", ["c2", "c4"])
def test_k2_handovers_in_flight_together(seq, cfg):
    cc.k2_handovers(seq, cfg)


def test_k3_submit_wait_mixed_sizes_and_kinds(seq):
    cc.k3_submit_wait(seq, "c2")


def test_finding3_destroy_completes_tickets_nobody_waited_for(seq):
    cc.finding3_destroy_completes_tickets(seq, "c2")


def test_k4_host_threads_one_handle(seq):
    cc.k4_threads_one_handle(seq, "c2", rounds=40)


def test_k5_host_threads_several_handles(seq, gnarly):
    cc.k5_threads_many_handles(seq, ProblemTemplate(gnarly, "body", gnarly_goals()), rounds=12)


def test_k6_errors_stay_with_their_thread(seq):
    cc.k6_errors_stay_with_their_thread(seq, "c2", rounds=40)


def test_k7_far_timeout_among_overlapping_calls(seq):
    cc.k7_far_timeout(seq, "c2")


def test_k8_graphs_of_two_streams_replayed_together(seq):
    cc.k8_graphs_of_two_streams(seq, "c2")


def test_k9_chip_filling_calls_together(seq):
    cc.k9_chip_filling_calls_together(seq, "c2")
