"""Ranked solves (tests/ranked_cases.py) on a real MI355X: HipSolver(device=0), torch tensors and streams, and the device-pointer entry captured through
torch.cuda.graph.  Graphs are destroyed before their handle."""
import pytest

import limit_cases as lc
import ranked_cases as rk
from oracle import orc
from test_gpu_sequences import TorchDevice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def shared_trigonometry():
    orc.set_trig_mode(1)
    yield
    orc.set_trig_mode(0)


@pytest.fixture
def ctx(templates, oracles, monkeypatch):
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return rk.Ctx(lambda t: HipSolver(t, device=0), TorchDevice(), templates, oracles, monkeypatch)


@pytest.mark.parametrize("name", sorted(rk.RANK0))
def test_rank0_is_the_plain_answer(ctx, name):
    rk.r1_rank0(ctx, name)


@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_every_island_in_order(ctx, cfg):
    if cfg == "c2":
        rk.r2_every_island(ctx)
    else:
        rk.r2_every_island(ctx, "c3", 3, dict(population=128, islands=4, max_steps=2, random_seed=8))


def test_ties_go_to_the_lower_island(ctx):
    rk.r2_ties(ctx)


def test_distinct_rows(ctx):
    rk.r3_distinct(ctx)


def test_equal_rows_keep_one(ctx):
    rk.r3_equal_rows(ctx)


def test_paths(ctx):
    rk.r4_paths(ctx)


def test_mixed_calls_on_one_handle_and_stream(ctx):
    rk.r5_mixed(ctx)


def test_refusals(ctx):
    rk.r6_refusals(ctx)


def test_unsupported_stays_unsupported(ctx):
    rk.r6_unsupported(ctx, lambda: lc.envelope_problems()[-1][2])


def test_device_entry_and_capture(ctx):
    rk.r7_device_and_graph(ctx)


def test_result_level(ctx):
    rk.r8_results(ctx, 256)
