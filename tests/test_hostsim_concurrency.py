"""The concurrency cases of tests/concurrency_cases.py on the host simulator (tests/hostsim): K1, K2, K3 and K7 in its overlap mode, one round per scheduler seed
(launches queued per stream, workgroups of different streams interleaved), K4 - K6 from real host threads.  Every test ends with the simulator's three counters
unmoved: no write out of bounds of a device block, nothing inside a capture that HIP would refuse, no divergent collective."""
import ctypes

import numpy as np
import pytest

import concurrency_cases as cc
import limit_cases as lc
from bio_ik_amd import ProblemTemplate
from bio_ik_amd.solver import HipSolver
from conftest import gnarly_goals
from oracle import orc
from test_hostsim_sequences import HostDevice, counters


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


def all_counters(lib):
    lib.hostsim_divergent_collectives.restype = ctypes.c_ulonglong
    two = counters(lib)
    return lambda: two() + (lib.hostsim_divergent_collectives(),)


@pytest.fixture
def seq(hostsim_lib, templates, oracles, monkeypatch, capfd):
    count = all_counters(hostsim_lib)
    before = count()
    s = cc.Concurrency(lambda t: HipSolver(t, lib=hostsim_lib), HostDevice(hostsim_lib), lc.Report(monkeypatch, capfd), monkeypatch, templates, oracles)
    yield s
    after = count()
    assert after[0] == before[0], "write out of bounds of a device block (see the [hostsim] lines on stderr)"
    assert after[1] == before[1], "something HIP refuses inside a capture (see the [hostsim] lines on stderr)"
    assert after[2] == before[2], "lanes met at different collectives (see the [hostsim] lines on stderr)"


def test_overlap_selftest(hostsim_lib):
    """the scheduler itself: two launches on two streams each log (stream, workgroup).  Under a seed the log interleaves, keeps each stream's order and is
    reproducible; another seed gives another order; with overlap off the order is strictly sequential; nothing runs before a wait asks for it, a fill ahead of a
    launch on its stream stays ahead, and captures are refused meanwhile"""
    dev = HostDevice(hostsim_lib)
    L = hostsim_lib
    L.hostsim_selftest_log.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.hostsim_selftest_enqueue.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    count = all_counters(L)
    c0 = count()
    blocks = 12
    sequential = [(7, b) for b in range(blocks)] + [(9, b) for b in range(blocks)]

    def run(seed):
        log = np.zeros(1 + 4 * blocks, dtype=np.int32)
        words = np.zeros(2, dtype=np.uint32)
        if seed is None:
            L.hostsim_selftest_log(7, 7, blocks, log.ctypes.data)
            L.hostsim_selftest_log(9, 9, blocks, log.ctypes.data)
        else:
            with dev.overlap(seed):
                L.hostsim_selftest_log(7, 7, blocks, log.ctypes.data)
                L.hostsim_selftest_log(9, 9, blocks, log.ctypes.data)
                L.hostsim_selftest_enqueue(7, words.ctypes.data)  # (a fill of words[0], then two workgroups that count in words[1])
                assert log[0] == 0 and words.tolist() == [0, 0], "something ran at its enqueue"
                assert L.hostsim_capture_begin(5) == -1, "a capture began in overlap mode"
            assert words.tolist() == [0xffffffff, 2]
        assert log[0] == 2 * blocks
        return [tuple(x) for x in log[1:].reshape(-1, 2).tolist()]
    assert run(None) == sequential
    before = dev.interleaved()
    a = run(3)
    assert dev.interleaved() > before
    assert sorted(a) == sorted(sequential) and a != sequential
    for s in (7, 9):
        assert [e for e in a if e[0] == s] == [e for e in sequential if e[0] == s], "a stream's workgroups out of order"
    switches = sum(1 for x, y in zip(a, a[1:]) if x[0] != y[0])
    assert switches >= 4, a
    assert run(3) == a
    assert run(4) != a
    assert run(None) == sequential
    assert L.hostsim_overlap_end() == -1  # (not on)
    assert count() == c0


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
    cc.k4_threads_one_handle(seq, "c2")


def test_k5_host_threads_several_handles(seq, gnarly):
    cc.k5_threads_many_handles(seq, ProblemTemplate(gnarly, "body", gnarly_goals()))


def test_k6_errors_stay_with_their_thread(seq):
    cc.k6_errors_stay_with_their_thread(seq, "c2")


def test_k7_far_timeout_among_overlapping_calls(seq):
    cc.k7_far_timeout(seq, "c2")
