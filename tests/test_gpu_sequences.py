"""The call sequences of tests/sequence_cases.py on a real MI355X: HipSolver(device=0), torch tensors, torch.cuda.Stream, and the captures of S4 through
torch.cuda.graph (single-stream, linear graphs).  Graphs are destroyed before their handle."""
import contextlib

import pytest

import limit_cases as lc
import sequence_cases as sq
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


class TorchBuf:
    def __init__(self, a):
        import torch
        self.t = torch.from_numpy(a).to("cuda:0")
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy()

    def zero(self):
        self.t.zero_()


class TorchDevice:
    def __init__(self):
        import torch
        self.torch = torch
        self.streams = {}

    def buf(self, a):
        return TorchBuf(a)

    def stream(self, i):
        if i not in self.streams:
            self.streams[i] = self.torch.cuda.Stream(self.torch.device("cuda", 0))
        return self.streams[i]

    def handle(self, s):
        return s.cuda_stream

    def on(self, s):
        return self.torch.cuda.stream(s)

    def sync(self):
        self.torch.cuda.synchronize()

    overlap_seeds = (None,)  # tests/concurrency_cases.py: on the device the overlap is real, nothing to seed

    def overlap(self, seed):
        """nothing synchronises between the enqueues inside"""
        return contextlib.nullcontext()

    def heavy_rounds(self, cfg):
        return None  # (every round)

    def interleaved(self):
        return None

    def sync_stream(self, s):
        s.synchronize()

    def capture(self, s, enqueue):
        g = self.torch.cuda.CUDAGraph()
        with self.torch.cuda.graph(g, stream=s):
            enqueue()
        return g

    def replay(self, g):
        g.replay()

    def replay_on(self, g, s):
        with self.torch.cuda.stream(s):
            g.replay()

    def destroy(self, g):
        g.reset()


@pytest.fixture
def seq(templates, oracles, monkeypatch, capfd):
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return sq.Sequences(lambda t: HipSolver(t, device=0), TorchDevice(), lc.Report(monkeypatch, capfd), monkeypatch, templates, oracles)


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
