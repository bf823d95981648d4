"""Base links (tests/base_link_cases.py) on the host simulator (tests/hostsim): the kernel bodies of the product stepped on the CPU against the long-double
restatement of the rule.  Run with -s for the worst error / bound ratios."""
import pytest

import base_link_cases as bc
import random_robot_cases as rr
from bio_ik_amd import abi
from bio_ik_amd.solver import HipSolver
from limit_cases import Report


WORKERS = 8  # (the simulator steps every lane of a solve on the calling thread: a whole solve runs in slices on eight threads, base_link_cases.sharded)


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


@pytest.fixture(scope="module")
def stats():
    s = rr.Stats()
    yield s
    print("\n[base links, hostsim] " + s.line())


@pytest.mark.parametrize("name", sorted(bc.function_cases()))
def test_function_level(make_solver, stats, name):
    bc.function_level(make_solver, name, stats, n=200)


def test_streamed_fitness(make_solver):
    bc.streamed(make_solver, lambda a: (a.ctypes.data, (lambda: a)))


def test_identity(make_solver, monkeypatch, capfd):
    bc.identity(make_solver, Report(monkeypatch, capfd))


def test_refusals(make_solver, hostsim_lib):
    bc.refusals(make_solver, hostsim_lib)


@pytest.mark.parametrize("fk", [abi.FK_EXACT, abi.FK_LINEAR], ids=["exact", "linear"])
@pytest.mark.parametrize("variant", ["tray", "apart", "aim"])
def test_whole_solve(make_solver, variant, fk):
    """16 reachable queries, 64 steps, four islands, dtwist 1e-5, bio2_memetic.  Measured on the host simulator (= the device, bit for bit), solved of 16:
    tray exact 15, linear 14; apart exact 16, linear 16; aim exact 16, linear
    16; the floor of the test is 8."""
    bc.whole_solve(make_solver, variant, fk=fk, workers=WORKERS)[0].close()


@pytest.mark.parametrize("kind", bc.TRAY_KINDS)
def test_whole_solve_tray(make_solver, kind):
    """"tray" under gd_r with four islands, ranked (k = 2), bounded (+-0.5 around the seed), with island_migration = 2, with island_sync = 1 and with a timeout of
    an hour (the bits of the call without), and under gd and gd_c.  Measured on the host simulator, solved of 16: gd_r 12, ranked 15 in row 0 (12 in row
    1), bounded 15, migration 16, island_sync 15, timeout 15 (floor 8); gd 12, gd_c 16 (no floor set: fitness and bits).  The gradient
    variants start 0.03 from their targets and are judged with dtwist = 2e-2 (base_link_cases.whole_solve says why)."""
    bc.whole_solve(make_solver, "tray", kind, workers=WORKERS)[0].close()


def test_mapping_independence(make_solver, monkeypatch, capfd):
    # (the simulator steps every lane on one CPU thread: two queries and two steps here; tests/test_gpu_base_link.py runs the whole-solve cases)
    bc.mapping_independence(make_solver, monkeypatch, Report(monkeypatch, capfd), variants=("tray",), steps=2, n=2, islands=2)
