"""ClearanceGoal (tests/clearance_cases.py) on a real MI355X: HipSolver(device=0) against the long-double restatement of the goal, and bit for bit against the host
simulator of the same kernel bodies (tests/hostsim/libbioik_hostsim.so) run in the same test.  Run with -s for the worst error / bound ratios."""
import numpy as np
import pytest

import clearance_cases as cc
import random_robot_cases as rr
from bio_ik_amd import abi

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
    print("\n[clearance, MI355X] " + s.line())


def hbm_arrays(a):
    import torch
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(a).to(dev)

    def fetch():
        torch.cuda.synchronize(dev)
        return t.cpu().numpy()
    return t.data_ptr(), fetch


@pytest.mark.parametrize("name", sorted(cc.function_cases()))
def test_function_level(make_solver, stats, name):
    cc.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    cc.streamed(make_solver, hbm_arrays)


def test_table_updates(make_solver, stats):
    from bio_ik_amd.solver import load_library
    cc.table_updates(make_solver, stats, load_library())


def test_refusals(make_solver):
    from bio_ik_amd.solver import load_library
    cc.refusals(make_solver, load_library())


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_whole_solve_and_simulator(make_solver, hostsim_lib, variant):
    """16 queries behind the column, 64 steps, four islands, dtwist 1e-5: the asserts of clearance_cases.verify_solve and, for "primary", of clearance_cases.steering
    (the counts found: tests/test_hostsim_clearance.py), and results and steps bit for bit those of the host simulator."""
    from bio_ik_amd.solver import HipSolver
    h, t, seeds, params, p, res = cc.whole_solve(make_solver, variant)
    sim = HipSolver(t, lib=hostsim_lib)
    _, want = cc.run(sim, t, variant, seeds, params)
    assert all(np.array_equal(a, b) for a, b in zip(res, want)), variant
    sim.close()
    h.close()


def test_mapping_independence(make_solver, monkeypatch):
    cc.mapping_independence(make_solver, monkeypatch)


def test_capture_replays_with_the_current_table(make_solver):
    """the device form of the solve captured into a hipGraph once: a replay equals the eager call; after bioik_problem_set_obstacles the SAME graph's next replay equals
    an eager call with the new table (the table's address never changes and its row count lives beside it in device memory)"""
    import torch
    t = cc.solve_template("primary")
    h = make_solver(t)
    seeds, params = cc.queries(t)
    n = seeds.shape[0]
    p = abi.default_solve_params(**cc.SOLVE)
    moved = cc.COLUMN + np.array([0.0, 0.1, 0.0, 0.02])
    want_old = h.solve_batch(p, seeds, params)
    for k in t.obstacle_tables():
        h.set_obstacles(k, moved[:5])
    want_new = h.solve_batch(p, seeds, params)
    assert not np.array_equal(want_old[0], want_new[0])
    for k, rows in t.obstacle_tables().items():
        h.set_obstacles(k, rows)
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
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(o, want_old))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue()
    for want in (want_old, want_new):
        for a in o:
            a.zero_()
        g.replay()
        torch.cuda.synchronize()  # (the replay is complete before the table changes: device-pointer solves are the caller's to wait for)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(o, want))
        for k in t.obstacle_tables():
            h.set_obstacles(k, moved[:5])
    del g
    h.close()
