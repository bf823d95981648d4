"""Base links (include/bioik_hip.h: BASE LINKS) at the Python boundary: the goal classes' accessors and keyword, what ProblemTemplate marshals, and the
struct_size rule of bioik_problem_desc through ctypes against the host simulator."""
import ctypes as C

import numpy as np
import pytest

from bio_ik_amd import (ConeGoal, DirectionGoal, LineGoal, LookAtGoal, MaxDistanceGoal, MinDistanceGoal, OrientationGoal, PlaneGoal, PoseGoal, PositionGoal,
                        ProblemTemplate, SideGoal, TouchGoal, abi, pr2_like)
from bio_ik_amd.solver import HipSolver

RW, LW = "r_wrist_roll_link", "l_wrist_roll_link"
LINK_GOALS = [PositionGoal, OrientationGoal, PoseGoal, LookAtGoal, MaxDistanceGoal, MinDistanceGoal, LineGoal, PlaneGoal, SideGoal, DirectionGoal, ConeGoal, TouchGoal]


@pytest.mark.parametrize("cls", LINK_GOALS, ids=lambda c: c.__name__)
def test_accessors_and_keyword(cls):
    g = cls(LW)
    assert g.getBaseLinkName() == "" and g.base_link_name() is None  # the world
    g.setBaseLinkName(RW)
    assert g.getBaseLinkName() == RW and g.base_link_name() == RW and g.getLinkName() == LW
    g = cls(LW, base_link=RW)
    assert g.getBaseLinkName() == RW
    assert np.array_equal(g.params(), cls(LW).params())  # the numbers of a goal do not change, only the frame they are read in


def test_constants():
    assert abi.MAX_HELD_FRAMES == 4
    assert abi.ProblemDesc.goal_base_link.offset == abi.ProblemDesc.fixed_joints.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(abi.ProblemDesc) == abi.ProblemDesc.goal_base_link.offset + C.sizeof(C.c_void_p)


def test_marshalling(hostsim_lib):
    m = pr2_like()
    world = ProblemTemplate(m, "all", [PoseGoal(RW), PoseGoal(LW)])
    assert not world.desc().goal_base_link  # NULL: no goal has a base
    t = ProblemTemplate(m, "all", [PoseGoal(RW), PoseGoal(LW, base_link=RW), PositionGoal(LW)])
    d = t.desc()
    assert d.struct_size == C.sizeof(abi.ProblemDesc) and [d.goal_base_link[i] for i in range(3)] == [-1, m.link_index(RW), -1]
    with pytest.raises(KeyError):
        ProblemTemplate(m, "all", [PoseGoal(LW, base_link="no_such_link")])
    # the base link is a tip of the problem and the joints of its chain are active variables: a goal on the left wrist alone has the left arm's seven variables
    # and the torso's, with the right wrist as its base also the right arm's
    alone = HipSolver(ProblemTemplate(m, "all", [PoseGoal(LW)]), lib=hostsim_lib)
    based = HipSolver(ProblemTemplate(m, "all", [PoseGoal(LW, base_link=RW)]), lib=hostsim_lib)
    assert list(alone.tip_links) == [m.link_index(LW)] and list(based.tip_links) == [m.link_index(LW), m.link_index(RW)]  # behind the goal's own link
    names = lambda h: sorted(m.variable_names[v] for v in h.active_variables)  # noqa: E731
    assert len(names(alone)) == 8 and not any(n.startswith("r_") for n in names(alone))
    assert len(names(based)) == 15 and sum(n.startswith("r_") for n in names(based)) == 7 and sum(n.startswith("l_") for n in names(based)) == 7
    assert based.P == 8  # bioik_goal_param_count does not change
    alone.close()
    based.close()


def test_struct_size_rule(hostsim_lib):
    """a caller whose struct_size ends in front of goal_base_link gets none (its based goal is a world goal: one tip); a size that ends inside the field is refused"""
    L = hostsim_lib
    m = pr2_like()
    t = ProblemTemplate(m, "all", [PoseGoal(LW, base_link=RW)])
    md, model = m.desc(), C.c_void_p()
    assert L.bioik_model_create(C.byref(md), 0, C.byref(model)) == abi.OK

    def create(size):
        d, prob = t.desc(), C.c_void_p()
        d.struct_size = size
        rc = L.bioik_problem_create(model, C.byref(d), C.byref(prob))
        tips = L.bioik_problem_tip_count(prob) if rc == abi.OK else None
        if rc == abi.OK:
            L.bioik_problem_destroy(prob)
        return rc, tips
    off = abi.ProblemDesc.goal_base_link.offset
    assert create(C.sizeof(abi.ProblemDesc)) == (abi.OK, 2)
    assert create(off) == (abi.OK, 1)
    for size in (off + 4, off - 8, C.sizeof(abi.ProblemDesc) + 8, 0):
        assert create(size) == (abi.ERR_INVALID_ARGUMENT, None), size
        assert b"struct_size" in L.bioik_last_error()
    L.bioik_model_destroy(model)


def test_python_plugin_tray(hostsim_shim):
    """a based goal through the Python plugin (bio_ik_amd/plugin.py -> the shim's goal records -> plugin_core.h): the plugin's default PoseGoal poses the right
    wrist in the world, the caller's PoseGoal the left wrist in the right wrist's frame, and a LookAtGoal behind it in the list arrives with its own fields"""
    from bio_ik_amd import BioIKKinematicsPlugin, BioIKKinematicsQueryOptions, LookAtGoal, MoveItErrorCodes
    from bio_ik_amd.robot import link_transform, quat_multiply, quat_rotate
    m = pr2_like()
    p = BioIKKinematicsPlugin(lib=hostsim_shim)
    assert p.initialize(m, "all", "base_footprint", [RW], 0.0, params={"gpu_population": 128, "gpu_max_steps": 128, "gpu_islands": 4, "random_seed": 2})
    gv = np.asarray(p._group_vars)
    lo, hi = np.asarray(m.var_min)[gv], np.asarray(m.var_max)[gv]
    target = m.default_positions()
    target[gv] = lo + (hi - lo) * (0.3 + 0.03 * np.arange(len(gv)))
    seed = target[gv] + 0.05 * (hi - lo)

    def relative(state):
        a, b = link_transform(m, m.link_index(RW), state), link_transform(m, m.link_index(LW), state)
        inv = np.array([-a[3], -a[4], -a[5], a[6]])
        return a, np.concatenate([quat_rotate(inv, b[:3] - a[:3]), quat_multiply(inv, b[3:])])
    A, R = relative(target)
    axis = np.array([1.0, 0.0, 0.0])
    opt = BioIKKinematicsQueryOptions()
    opt.goals = [PoseGoal(LW, R[:3], R[3:], base_link=RW), LookAtGoal(LW, axis, R[:3] + 0.3 * quat_rotate(R[3:], axis), weight=0.5, base_link=RW)]
    solution, code = [], MoveItErrorCodes()
    assert p.searchPositionIK([A], list(seed), 600.0, solution, code, options=opt) is True and code.val == MoveItErrorCodes.SUCCESS
    state = m.default_positions()
    state[gv] = solution
    a, r = relative(state)
    # (every twist component below dtwist = 1e-5: the position errors below sqrt(3) dtwist)
    assert np.linalg.norm(r[:3] - R[:3]) < 2e-5 and np.linalg.norm(a[:3] - A[:3]) < 2e-5, (r, R)
    assert np.linalg.norm(link_transform(m, m.link_index(LW), state)[:3] - R[:3]) > 0.1  # (read in the world frame the goal would put the left wrist elsewhere)
