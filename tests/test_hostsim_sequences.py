"""The call sequences of tests/sequence_cases.py on the host simulator (tests/hostsim), whose device memory is guarded (a redzone before and behind every
block: a write out of bounds is counted) and whose streams can be captured (fills, copies and launches recorded by value and replayed; what HIP would refuse
inside a capture is counted).  Every test ends with neither count moved."""
import contextlib
import ctypes

import numpy as np
import pytest

import limit_cases as lc
import sequence_cases as sq
from bio_ik_amd.solver import HipSolver
from oracle import orc


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


class HostBuf:
    def __init__(self, a):
        self.a = a
        self.ptr = a.ctypes.data

    def get(self):
        return self.a.copy()

    def zero(self):
        self.a[...] = 0


class HostDevice:
    """device pointers are host pointers; streams are small integers; graphs are the simulator's recorded captures"""

    def __init__(self, lib):
        self.L = lib
        lib.hostsim_capture_begin.argtypes = [ctypes.c_void_p]
        lib.hostsim_capture_end.argtypes = [ctypes.c_void_p]
        lib.hostsim_capture_end.restype = ctypes.c_longlong
        lib.hostsim_graph_replay.argtypes = [ctypes.c_longlong]
        lib.hostsim_graph_destroy.argtypes = [ctypes.c_longlong]
        lib.hostsim_overlap_begin.argtypes = [ctypes.c_ulonglong]
        lib.hostsim_overlap_interleaved.restype = ctypes.c_ulonglong

    overlap_seeds = (11, 12, 13, 14)  # tests/concurrency_cases.py: the scheduler's seeds a case runs under

    @contextlib.contextmanager
    def overlap(self, seed):
        """the simulator's overlap mode: what is enqueued inside is queued per stream and run, workgroups of different streams interleaved by the
        scheduler seeded with `seed`, where the library waits for a stream and -- all that is left -- at the end"""
        assert self.L.hostsim_overlap_begin(seed) == 0
        try:
            yield
        finally:
            assert self.L.hostsim_overlap_end() == 0

    def heavy_rounds(self, cfg):
        """the rounds of a window that S1's pair of calls takes part in: 800 units and more, half a minute per round in the simulator on c2 and more on c4"""
        return (0, 1) if cfg == "c2" else (0,)

    def interleaved(self):
        """workgroups run so far while a launch of another stream was part-way through its grid"""
        return self.L.hostsim_overlap_interleaved()

    def sync_stream(self, s):
        pass

    def buf(self, a):
        return HostBuf(a)

    def stream(self, i):
        return i

    def handle(self, s):
        return s

    def on(self, s):
        return contextlib.nullcontext()

    def sync(self):
        pass

    def capture(self, s, enqueue):
        assert self.L.hostsim_capture_begin(s) == 0
        try:
            enqueue()
        finally:
            g = self.L.hostsim_capture_end(s)
        assert g > 0
        return g

    def replay(self, g):
        assert self.L.hostsim_graph_replay(g) == 0

    def destroy(self, g):
        assert self.L.hostsim_graph_destroy(g) == 0


def counters(lib):
    for f in (lib.hostsim_guard_violations, lib.hostsim_capture_violations):
        f.restype = ctypes.c_ulonglong
    return lambda: (lib.hostsim_guard_violations(), lib.hostsim_capture_violations())


@pytest.fixture
def seq(hostsim_lib, templates, oracles, monkeypatch, capfd):
    count = counters(hostsim_lib)
    before = count()
    s = sq.Sequences(lambda t: HipSolver(t, lib=hostsim_lib), HostDevice(hostsim_lib), lc.Report(monkeypatch, capfd), monkeypatch, templates, oracles)
    yield s
    after = count()
    assert after[0] == before[0], "write out of bounds of a device block (see the [hostsim] lines on stderr)"
    assert after[1] == before[1], "something HIP refuses inside a capture (see the [hostsim] lines on stderr)"


def test_guard_and_capture_selftest(hostsim_lib):
    """the detectors themselves: a byte written just past a block is reported, its last byte is not; a captured fill and launch run once per replay, not at
    capture, and run at once on a stream that is not being captured"""
    count = counters(hostsim_lib)
    g0, c0 = count()
    hostsim_lib.hostsim_selftest_write(ctypes.c_ulonglong(100), ctypes.c_ulonglong(99))
    assert count()[0] == g0
    hostsim_lib.hostsim_selftest_write(ctypes.c_ulonglong(100), ctypes.c_ulonglong(100))
    assert count()[0] == g0 + 1
    dev = HostDevice(hostsim_lib)
    hostsim_lib.hostsim_selftest_enqueue.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    words = np.zeros(2, dtype=np.uint32)
    g = dev.capture(7, lambda: hostsim_lib.hostsim_selftest_enqueue(7, words.ctypes.data))
    assert words.tolist() == [0, 0]
    dev.replay(g)
    assert words.tolist() == [0xffffffff, 2]
    words[0] = 5
    dev.replay(g)
    assert words.tolist() == [0xffffffff, 4]
    dev.destroy(g)
    hostsim_lib.hostsim_selftest_enqueue(7, words.ctypes.data)  # (not capturing: at once)
    assert words.tolist() == [0xffffffff, 6]
    assert count()[1] == c0


def test_s1_finding1_eager_write_past_the_scratch(seq):
    sq.s1_finding1(seq, "c2")


def test_s2_reverse_order_and_reduction_kinds(seq):
    sq.s2_reverse_and_kinds(seq, "c2")


@pytest.mark.parametrize("cfg", ["c2", "c4"])
def test_s3_interleaved_kinds(seq, cfg):
    sq.s3_interleaved(seq, cfg)


def test_s4_graphs_on_one_stream(seq):
    sq.s4_captures(seq, "c2")


def test_s5_two_streams_of_one_handle(seq):
    sq.s5_two_streams(seq, "c2")
