"""Base links (tests/base_link_cases.py) on a real MI355X: HipSolver(device=0) against the long-double restatement of the rule, and bit for bit against the host
simulator of the same kernel bodies (tests/hostsim/libbioik_hostsim.so) run in the same test.  Run with -s for the worst error / bound ratios."""
import numpy as np
import pytest

import base_link_cases as bc
import random_robot_cases as rr
from bio_ik_amd import abi
from limit_cases import Report

pytestmark = pytest.mark.gpu


@pytest.fixture
def make_solver():
    from bio_ik_amd.solver import HipSolver, device_count
    assert device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return lambda t: HipSolver(t, device=0)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[base links, MI355X] " + s.line())


def hbm_arrays(a):
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(a).to(dev)

    def fetch():
        torch.cuda.synchronize(dev)
        return t.cpu().numpy()
    return t.data_ptr(), fetch


@pytest.mark.parametrize("name", sorted(bc.function_cases()))
def test_function_level(make_solver, hostsim_lib, stats, name):
    from bio_ik_amd.solver import HipSolver
    bc.function_level(make_solver, name, stats, n=200)
    # ... and the device's fitness bit for bit the simulator's
    model, group, goals = bc.function_cases()[name]
    t = bc.ProblemTemplate(model, group, goals)
    h, sim = make_solver(t), HipSolver(t, lib=hostsim_lib)
    rng = np.random.default_rng(1)
    seed = np.asarray(model.default_positions(), dtype=np.float64)
    genes = np.ascontiguousarray(rng.uniform(-1, 1, size=(50, h.D)))
    for fk in (abi.FK_EXACT, abi.FK_LINEAR):
        assert np.array_equal(h.fitness(fk, seed, t.pack_params(), genes, genes[0])[0], sim.fitness(fk, seed, t.pack_params(), genes, genes[0])[0]), (name, fk)
    sim.close()
    h.close()


def test_streamed_fitness(make_solver):
    bc.streamed(make_solver, hbm_arrays)


def test_identity(make_solver, monkeypatch, capfd):
    bc.identity(make_solver, Report(monkeypatch, capfd))


def test_refusals(make_solver):
    from bio_ik_amd.solver import load_library
    bc.refusals(make_solver, load_library())


def against_simulator(hostsim_lib, kind, h, t, seeds, params, p, bounds, res):
    """every row of the device's answer against the host simulator's, bit for bit (the simulator solves the call in slices on eight threads, each announced by
    its global offset: base_link_cases.sharded)"""
    from bio_ik_amd.solver import HipSolver
    want = bc.simulator_answer(lambda: HipSolver(t, lib=hostsim_lib), kind, p, seeds, params, bounds)
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(res, want)), kind
    h.close()


@pytest.mark.parametrize("fk", [abi.FK_EXACT, abi.FK_LINEAR], ids=["exact", "linear"])
@pytest.mark.parametrize("variant", ["tray", "apart", "aim"])
def test_whole_solve_and_simulator(make_solver, hostsim_lib, variant, fk):
    """16 reachable queries, 64 steps, four islands, dtwist 1e-5, bio2_memetic: the asserts of base_link_cases.verify_solve (the counts measured on the host
    simulator stand in tests/test_hostsim_base_link.py; the floor is 8), and results and steps bit for bit those of the host simulator."""
    against_simulator(hostsim_lib, "plain", *bc.whole_solve(make_solver, variant, fk=fk))


@pytest.mark.parametrize("kind", bc.TRAY_KINDS)
def test_whole_solve_tray_and_simulator(make_solver, hostsim_lib, kind):
    """"tray" under gd_r, gd, gd_c, ranked (k = 2), bounded, island_migration = 2, island_sync = 1 and a timeout of an hour: base_link_cases.verify_solve on the
    device's answer, and all of it bit for bit the host simulator's"""
    against_simulator(hostsim_lib, kind, *bc.whole_solve(make_solver, "tray", kind))


def test_mapping_independence(make_solver, monkeypatch, capfd):
    bc.mapping_independence(make_solver, monkeypatch, Report(monkeypatch, capfd))


def test_capture_and_two_replays(make_solver):
    """the device form of the "tray" solve captured into a hipGraph once and replayed twice: every replay equals the eager call"""
    import torch
    t = bc.solve_template("tray")
    h = make_solver(t)
    seeds, params = bc.reachable_queries(t, h)
    n = seeds.shape[0]
    p = abi.default_solve_params(**bc.SOLVE)
    want = h.solve_batch(p, seeds, params)
    dev = torch.device("cuda", 0)
    ds, dp = torch.from_numpy(seeds).to(dev), torch.from_numpy(params).to(dev)
    o = (torch.empty((n, h.V), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
         torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    s = torch.cuda.Stream(dev)

    def enqueue():
        h.solve_batch_device(p, n, ds.data_ptr(), dp.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), s.cuda_stream)
    with torch.cuda.stream(s):
        enqueue()  # (the eager call of the same plan that sizes the scratch, include/bioik_hip.h)
    torch.cuda.synchronize()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(o, want))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue()
    for i in range(2):
        for a in o:
            a.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(o, want)), i
    del g
    h.close()
