"""SelfClearanceGoal in the layers above the kernel (no GPU: the host simulator stands behind HipSolver and the plugin shim): the constants of abi.py against the header,
the goal class and its numpy evaluate against the long-double restatement of tests/self_clearance_cases.py, the template's goal_base_link row, and the Python plugin:
one call whose answer is clear by the margin, and two requests that differ only in the other link compiled into two problems."""
import os
import re

import numpy as np

import base_link_cases as bl
import clearance_cases as cc
import self_clearance_cases as sc
from bio_ik_amd import BioIKKinematicsPlugin, MoveItErrorCodes, PositionGoal, ProblemTemplate, SelfClearanceGoal, abi
from bio_ik_amd.goals import BioIKKinematicsQueryOptions
from bio_ik_amd.robot import link_transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_against_the_header(hostsim_lib):
    text = open(os.path.join(ROOT, "include", "bioik_hip.h")).read()
    assert int(re.search(r"BIOIK_GOAL_SELF_CLEARANCE = (\d+)", text).group(1)) == abi.GOAL_SELF_CLEARANCE == 20
    assert int(re.search(r"BIOIK_GOAL_CLEARANCE = (\d+)", text).group(1)) == abi.GOAL_CLEARANCE == 19
    assert int(re.search(r"BIOIK_GOAL_TYPE_COUNT = (\d+)", text).group(1)) == 18 and 18 not in abi.GOAL_PARAM_COUNT  # opcode 18 stays unknown
    assert abi.GOAL_PARAM_COUNT[abi.GOAL_SELF_CLEARANCE] == 1 == hostsim_lib.bioik_goal_param_count(20) and hostsim_lib.bioik_goal_param_count(18) == -1
    assert int(re.search(r"#define BIOIK_ABI_VERSION (\d+)", text).group(1)) == 6 == hostsim_lib.bioik_abi_version()


def test_goal_class():
    g = SelfClearanceGoal(sc.RF, sc.LF, 0.03, weight=0.7)
    assert g.opcode == 20 and g.link_name() == sc.RF and g.getWeight() == 0.7 and not g.isSecondary()
    assert g.getOtherLinkName() == sc.LF == g.getBaseLinkName() == g.base_link_name() and np.array_equal(g.params(), [0.03]) and g.getMargin() == 0.03
    g.setOtherLinkName(sc.LW)
    assert g.getBaseLinkName() == sc.LW
    g.setBaseLinkName(sc.RW), g.setMargin(0.5)
    assert g.getOtherLinkName() == sc.RW and g.params()[0] == 0.5
    d = SelfClearanceGoal()
    assert d.base_link_name() is None and d.params()[0] == 0.0 and d.getWeight() == 1.0


def test_numpy_evaluate_against_the_restatement():
    """goals.SelfClearanceGoal.evaluate (float64, unfused) against the long-double restatement on random pairs of frames, unit quaternions and not: up to rounding"""
    rng = np.random.default_rng(2)
    pts = np.hstack([rng.uniform(-0.1, 0.1, (5, 3)), rng.uniform(0, 0.05, (5, 1))])
    obs = np.hstack([rng.uniform(-0.1, 0.1, (9, 3)), rng.uniform(0.1, 0.4, (9, 1))])
    g = SelfClearanceGoal("x", "y", 0.02)
    hits = 0
    for k in range(50):
        fr = []
        for scale in ((1.0, 1.0) if k % 2 else (1.1, 0.93)):
            q = rng.normal(size=4)
            fr.append(np.concatenate([rng.uniform(-0.3, 0.3, 3), q / np.linalg.norm(q) * scale]))
        b, a = fr
        p, q = bl.relative(a[None, :3], a[None, 3:], b[None, :3], b[None, 3:])
        pen, _, _ = cc.pair_penetrations(0.02, p, q, pts, obs)
        want = float((pen * pen).sum())
        got = g.evaluate(b, a, pts, obs)
        assert abs(got - want) <= 1e-13 * (1 + want), (k, got, want)
        hits += want > 0
    assert 5 < hits
    assert SelfClearanceGoal("x", "y", -1.0).evaluate(b, a, pts, obs) == 0.0 and g.evaluate(b, a, pts, np.zeros((0, 4))) == 0.0


def test_template_marshals_the_other_link(hostsim_lib):
    from bio_ik_amd.solver import HipSolver
    m = sc.solve_model()
    t = ProblemTemplate(m, "all", [PositionGoal(sc.RW), SelfClearanceGoal(sc.RF, sc.LF, 0.01)])
    d = t.desc()
    assert [d.goal_base_link[i] for i in range(2)] == [-1, m.link_index(sc.LF)] and d.goals[1].type == 20 and d.goals[1].link == m.link_index(sc.RF)
    assert t.param_count == 3 + 1 and t.pack_params()[3] == 0.01 and t.obstacle_tables() == {}
    h = HipSolver(t, lib=hostsim_lib)
    assert m.link_index(sc.RF) in h.tip_links and m.link_index(sc.LF) in h.tip_links and h.P == 4
    h.close()


def test_python_plugin(hostsim_shim):
    """bio_ik_amd.plugin over the plugin core: the default PoseGoal poses the right wrist where a configuration clear by 4 cm has it, the caller's SelfClearanceGoal keeps
    the forearms 2 cm apart.  Then the same request with ANOTHER other link: a second compiled problem."""
    m = sc.solve_model()
    m.add_collision_points(sc.LE, [[0.0, 0.0, 0.0]], [0.05])
    plugin = BioIKKinematicsPlugin(lib=hostsim_shim)
    assert plugin.initialize(m, "all", "base_footprint", [sc.RW], 0.0, params={"gpu_population": 64, "gpu_max_steps": 64, "random_seed": 3, "gpu_islands": 4})
    gv = np.asarray(plugin._group_vars)
    x = None
    # a configuration whose forearms are clear by 4 cm, found by rejection sampling: an answer exists
    rng = np.random.default_rng(4)
    lo, hi = np.asarray(m.var_min), np.asarray(m.var_max)
    while x is None or sc.forearm_depth(m, x[None], 0.04)[0] > 0.0:
        x = m.default_positions()
        x[gv] = (lo + (hi - lo) * rng.random(m.n_variables))[gv]
    pose = link_transform(m, m.link_index(sc.RW), x)

    def ask(other):
        opt = BioIKKinematicsQueryOptions()
        opt.goals = [SelfClearanceGoal(sc.RF, other, 0.02)]
        solution, code = [], MoveItErrorCodes()
        ok = plugin.searchPositionIK([pose], list(x[gv] + 0.1), 600.0, solution, code, options=opt)
        y = m.default_positions()
        if ok:
            y[gv] = solution
        return ok, y
    ok, y = ask(sc.LF)
    assert ok and sc.forearm_depth(m, y[None], 0.02)[0] < 1e-5 + 1e-12  # (the success rule: weighted cost < dtwist^2, so no pair deeper than dtwist)
    # the same request with the left elbow as the other link solves too; with a link that carries NO points it is refused when its problem is compiled -- a cache that
    # did not tell the pairs apart would hand it the forearms' problem and solve
    assert ask(sc.LE)[0]
    try:
        ok3 = ask(sc.LW)[0]
    except Exception as e:  # noqa: BLE001
        ok3 = False
        assert "no collision points" in str(e), e
    assert not ok3
    assert ask(sc.LF)[0]
