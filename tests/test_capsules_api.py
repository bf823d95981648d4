"""Capsules in the layers above the kernel (no GPU: the host simulator stands behind HipSolver): the descriptor and its struct_size forms, every refusal with its
message, the robot model's setters, the URDF path, and the Python evaluate() methods against the simulator and against the long-double restatement of
tests/capsule_cases.py."""
import ctypes as Ct
import os
import re

import numpy as np
import pytest

import capsule_cases as cap
import clearance_cases as cc
import self_clearance_cases as sc
import touch_cases as tc
import touch_disk_cases as td
from bio_ik_amd import ClearanceGoal, PoseGoal, ProblemTemplate, SelfClearanceGoal, TouchGoal, abi, load_urdf, pr2_like, solver
from bio_ik_amd.goals import segment_point_d2, segment_segment_d2
from bio_ik_amd.robot import link_transform
from bio_ik_amd.solver import HipSolver
from np_fk import LD
from test_touch_goal_api import URDF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIP, RW, LW = cap.TIP, cap.RW, cap.LW
ROW = [0.01, 0.02, -0.03, 0.04, 0.2, 0.0, 0.1]


@pytest.fixture
def make_solver(hostsim_lib):
    return lambda t: HipSolver(t, lib=hostsim_lib)


def refused(make_solver, lib, template, code, *words):
    try:
        make_solver(template)
    except solver.BioIKError as e:
        assert e.code == code and all(w in str(e) and w in lib.bioik_last_error().decode() for w in words), (code, words, e.code, str(e))
    else:
        raise AssertionError("accepted: %s %s" % (code, words))


def test_constants_against_the_header(hostsim_lib):
    text = open(os.path.join(ROOT, "include", "bioik_hip.h")).read()
    assert int(re.search(r"#define BIOIK_MAX_LINK_CAPSULES (\d+)", text).group(1)) == abi.MAX_LINK_CAPSULES == 64
    assert int(re.search(r"#define BIOIK_ABI_VERSION (\d+)", text).group(1)) == 6 == hostsim_lib.bioik_abi_version()
    # no new opcode: 21 and 18 stay unknown
    assert hostsim_lib.bioik_goal_param_count(21) == -1 and hostsim_lib.bioik_goal_param_count(18) == -1 and 21 not in abi.GOAL_PARAM_COUNT
    names = [f[0] for f in abi.ModelDesc._fields_]
    assert names[-4:] == ["link_disk_first", "link_disks", "link_capsule_first", "link_capsules"]
    assert re.search(r"link_disks;.*?link_capsule_first;.*?link_capsules;.*?\} bioik_model_desc;", text, re.S)


def test_robot_setters():
    m = pr2_like()
    m.add_collision_capsules(TIP, [ROW])  # an identity origin: the row untouched, the filling zero added
    assert np.array_equal(m.collision_capsules(TIP), [ROW + [0.0]])
    m.add_collision_capsule(TIP, 0.05, 0.3)  # centred, along z; `length` is the segment's
    assert np.array_equal(m.collision_capsules(TIP)[1], [0, 0, -0.15, 0.05, 0, 0, 0.15, 0])
    s = np.sqrt(0.5)
    m.add_collision_capsule(LW, 0.02, 0.2, (0.5, 0.0, 0.0, s, 0.0, 0.0, s))  # a quarter turn about x, then +0.5 x: z -> -y
    assert np.allclose(m.collision_capsules(LW), [(0.5, 0.1, 0.0, 0.02, 0.5, -0.1, 0.0, 0.0)], atol=1e-15, rtol=0)
    assert len(m.collision_capsules("base_link")) == 0
    for bad in ([0, 0, 0, -0.1, 1, 0, 0], [0, 0, np.nan, 0.1, 1, 0, 0], [0, 0, 0, np.inf, 1, 0, 0], [1, 2, 3, 0.1, 1, 2, 3], [0, 0, 0, 0.1, 1, 0, 0, 0.5]):
        with pytest.raises(ValueError):
            m.add_collision_capsules(TIP, [bad])
    with pytest.raises(ValueError, match="sphere"):
        m.add_collision_capsule(TIP, 0.1, 0.0)
    k = m.arrays()
    link = m.link_index(TIP)
    assert k["link_capsule_first"][link + 1] - k["link_capsule_first"][link] == 2 and k["link_capsule_first"][-1] == 3 and k["link_capsules"].shape == (3, 8)
    d = m.desc()
    assert d.link_capsule_first and d.link_capsules and d.struct_size == Ct.sizeof(abi.ModelDesc)
    d = pr2_like().desc()
    assert not d.link_capsule_first and not d.link_capsules


def test_invalid_rows_are_refused_by_the_library(hostsim_lib):
    """the Python setters refuse them too, so the rows are put into the descriptor behind their back"""
    m = pr2_like()
    m.add_collision_capsules(TIP, [ROW])
    first = np.zeros(m.n_links + 1, dtype=np.int32)
    first[m.link_index(TIP) + 1:] = 1
    for row, word in (((0, np.nan, 0, 0.1, 1, 0, 0, 0), "not finite"), ((0, 0, 0, np.inf, 1, 0, 0, 0), "not finite"), ((0, 0, 0, 0.1, 1, -np.inf, 0, 0), "not finite"),
                      ((0, 0, 0, -0.1, 1, 0, 0, 0), "radius"), ((0, 0, 0, -1.0, 1, 0, 0, 0), "radius"), ((1, 2, 3, 0.1, 1, 2, 3, 0), "a sphere is a point row"),
                      ((0, 0, 0, 0.1, 1, 0, 0, 2.0), "eighth")):
        d = m.desc()
        bad = np.array([row], dtype=np.float64)
        d.link_capsule_first, d.link_capsules = abi.iptr(first), abi.dptr(bad)
        rc, text = td.model_create(hostsim_lib, d)
        assert rc == abi.ERR_INVALID_ARGUMENT and "capsule" in text and word in text, (row, rc, text)
    for spoil in ("first", "rows", "start", "order"):
        d = m.desc()
        f = first.copy()
        if spoil == "first":
            d.link_capsule_first = None
        elif spoil == "rows":
            d.link_capsules = None
        elif spoil == "start":
            f[0] = 1
            d.link_capsule_first = abi.iptr(f)
        else:
            f[-1] = 0
            d.link_capsule_first = abi.iptr(f)
        assert td.model_create(hostsim_lib, d)[0] == abi.ERR_INVALID_ARGUMENT, spoil


def test_struct_size_forms(hostsim_lib):
    """the full size carries the capsules; a size that ends in front of the new pair is a caller of the previous header and gets none (its disks and points are
    there); the two earlier sizes as before; a size inside a pair or beyond the struct is refused"""
    lib = hostsim_lib
    m = pr2_like()
    m.add_collision_capsules(TIP, [ROW])
    m.add_collision_box(LW, tc.BOX)
    M = abi.ModelDesc
    goal_c, goal_b = [ClearanceGoal(TIP, 0.0)], [TouchGoal(LW, (0, 0, 0), (0, 0, 1))]
    for size, ok_capsule, ok_box in ((Ct.sizeof(M), True, True), (M.link_capsule_first.offset, False, True), (M.link_disk_first.offset, False, True), (M.link_point_first.offset, False, False)):
        d = m.desc()
        d.struct_size = size
        handle = Ct.c_void_p()
        assert lib.bioik_model_create(Ct.byref(d), 0, Ct.byref(handle)) == abi.OK, lib.bioik_last_error().decode()
        for goals, group, ok in ((goal_c, "right_arm", ok_capsule), (goal_b, "left_arm", ok_box)):
            pd, prob = ProblemTemplate(m, group, goals).desc(), Ct.c_void_p()
            rc = lib.bioik_problem_create(handle, Ct.byref(pd), Ct.byref(prob))
            assert (rc == abi.OK) == ok, (size, rc, lib.bioik_last_error().decode())
            if ok:
                lib.bioik_problem_destroy(prob)
            else:
                assert rc == abi.ERR_INVALID_ARGUMENT and "no collision points" in lib.bioik_last_error().decode()
        lib.bioik_model_destroy(handle)
    for size in (M.link_capsule_first.offset + 4, M.link_capsule_first.offset + 8, M.link_disk_first.offset + 8, Ct.sizeof(M) + 8, Ct.sizeof(M) + 16):
        d = m.desc()
        d.struct_size = size
        assert td.model_create(lib, d)[0] == abi.ERR_INVALID_ARGUMENT, size


def test_caps_and_refusals(make_solver, hostsim_lib):
    lib = hostsim_lib
    K, P, O = abi.MAX_LINK_CAPSULES, abi.MAX_TOUCH_POINTS, abi.MAX_OBSTACLES
    shapes = cap.with_shapes
    # opcode 19: the three caps with their messages, the caps themselves accepted
    refused(make_solver, lib, ProblemTemplate(shapes(pr2_like(), TIP, 0, K + 1, 1), "right_arm", [ClearanceGoal(TIP)]), abi.ERR_UNSUPPORTED, "ClearanceGoal", "BIOIK_MAX_LINK_CAPSULES")
    refused(make_solver, lib, ProblemTemplate(shapes(pr2_like(), TIP, P - 1, 2, 1), "right_arm", [ClearanceGoal(TIP)]), abi.ERR_UNSUPPORTED, "ClearanceGoal", "BIOIK_MAX_TOUCH_POINTS")
    make_solver(ProblemTemplate(shapes(pr2_like(), TIP, P - K, K, 1), "right_arm", [ClearanceGoal(TIP)])).close()
    # opcode 20: either link, the message naming the goal, the link and the constant
    goal = [SelfClearanceGoal(RW, LW, 0.0)]
    pair = lambda a, b: ProblemTemplate(shapes(shapes(pr2_like(), RW, *a, 1), LW, *b, 2), "all", goal)  # noqa: E731
    refused(make_solver, lib, pair((1, K + 1), (1, 0)), abi.ERR_UNSUPPORTED, "goal 0", "the goal's link", "BIOIK_MAX_LINK_CAPSULES")
    refused(make_solver, lib, pair((1, 0), (0, K + 1)), abi.ERR_UNSUPPORTED, "goal 0", "the other link", "BIOIK_MAX_LINK_CAPSULES")
    refused(make_solver, lib, pair((P, 1), (1, 0)), abi.ERR_UNSUPPORTED, "goal 0", "the goal's link", "BIOIK_MAX_TOUCH_POINTS")
    refused(make_solver, lib, pair((1, 0), (O, 1)), abi.ERR_UNSUPPORTED, "goal 0", "the other link", "BIOIK_MAX_OBSTACLES")
    # TouchGoal: a capsule counts as two points
    refused(make_solver, lib, ProblemTemplate(shapes(pr2_like(), TIP, P - 1, 1, 1), "right_arm", [TouchGoal(TIP)]), abi.ERR_UNSUPPORTED, "TouchGoal", "BIOIK_MAX_TOUCH_POINTS")
    make_solver(ProblemTemplate(shapes(pr2_like(), TIP, P - 2, 1, 1), "right_arm", [TouchGoal(TIP)])).close()
    # a link with nothing stays "no collision points"; a link that carries only capsules is accepted by both opcodes
    refused(make_solver, lib, ProblemTemplate(pr2_like(), "right_arm", [ClearanceGoal(TIP)]), abi.ERR_INVALID_ARGUMENT, "no collision points")
    refused(make_solver, lib, pair((0, 0), (0, 1)), abi.ERR_INVALID_ARGUMENT, "goal 0", "the goal's link has no collision points")
    refused(make_solver, lib, pair((0, 1), (0, 0)), abi.ERR_INVALID_ARGUMENT, "goal 0", "the other link has no collision points")
    make_solver(ProblemTemplate(shapes(pr2_like(), TIP, 0, 1, 1), "right_arm", [ClearanceGoal(TIP)])).close()
    make_solver(pair((0, 1), (0, 1))).close()
    # capsules beside disks, or beside a marker row: refused with the present messages
    for spoil, word in (("disks", "disks"), ("marker", "radius -1")):
        m = shapes(shapes(pr2_like(), RW, 1, 1, 1), LW, 1, 1, 2)
        if spoil == "disks":
            m.add_collision_cylinder(RW, 0.03, 0.1)
        else:
            m.add_collision_unsupported(RW, "cylinder")
        refused(make_solver, lib, ProblemTemplate(m, "all", goal), abi.ERR_UNSUPPORTED, "goal 0", word)
        refused(make_solver, lib, ProblemTemplate(m, "right_arm", [ClearanceGoal(RW)]), abi.ERR_UNSUPPORTED, "ClearanceGoal", word)
    # a PoseGoal on a model with capsules: accepted, and in the lean flavour as before
    make_solver(ProblemTemplate(shapes(pr2_like(), TIP, 0, 2, 1), "right_arm", [PoseGoal(TIP)])).close()


def test_urdf_cylinder_as_its_bounding_capsule(make_solver, hostsim_lib):
    def model():
        m = load_urdf(URDF)
        m.add_group("g", joints=["j1", "j2"], tips=["rod"])
        return m
    goal = [ClearanceGoal("rod", 0.01, [[0.2, 0.0, 0.0, 0.1]])]
    m = model()
    refused(make_solver, hostsim_lib, ProblemTemplate(m, "g", goal), abi.ERR_UNSUPPORTED, "radius -1")  # as the reader leaves it: a marker
    rod = m.link_index("rod")
    m.resolve_collision_solids("rod", cylinders="capsule")
    # the same radius, the segment the whole axis: contains the cylinder, overshoots by r at each end
    assert np.array_equal(m.collision_capsules("rod"), [(0, 0, -0.1, 0.01, 0, 0, 0.1, 0)])
    assert len(m.collision_points("rod")) == 0 and len(m.collision_disks("rod")) == 0 and m.link_unsupported.get(rod, []) == [] and rod not in m.link_solids
    make_solver(ProblemTemplate(m, "g", goal)).close()
    d = model()
    d.resolve_collision_solids()  # the default still yields disks, which both clearance goals refuse
    assert len(d.collision_disks("rod")) == 2 and len(d.collision_capsules("rod")) == 0
    refused(make_solver, hostsim_lib, ProblemTemplate(d, "g", goal), abi.ERR_UNSUPPORTED, "disks")
    with pytest.raises(ValueError):
        model().resolve_collision_solids(cylinders="spheres")
    o = load_urdf(URDF.replace('<link name="rod"><collision>', '<link name="rod"><collision><origin xyz="0.1 0 0" rpy="1.5707963267948966 0 0"/>'))
    o.resolve_collision_solids(cylinders="capsule")
    assert np.allclose(o.collision_capsules("rod"), [(0.1, 0.1, 0, 0.01, 0.1, -0.1, 0, 0)], atol=1e-15, rtol=0)


def test_numpy_distances_against_the_restatement():
    """goals.segment_point_d2 / segment_segment_d2 (float64, the device's formula unfused) against the long-double distances of tests/capsule_cases.py, within the
    conditioning term of its docstring; a collapsed segment counts as its first end, and nothing is ever NaN"""
    rng = np.random.default_rng(5)
    for k in range(400):
        a, b, c, d = rng.uniform(-0.3, 0.3, size=(4, 3))
        if k % 4 == 1:  # near parallel
            d = c + (b - a) * rng.uniform(0.5, 1.5) + rng.normal(size=3) * 10.0 ** rng.uniform(-12, -1)
        if k % 4 == 2:  # exactly parallel
            d = c + (b - a)
        A, B, Cc, D = (np.asarray(x, dtype=LD) for x in (a, b, c, d))
        want = float(cap.segment_segment(A, B, Cc, D))
        got = np.sqrt(segment_segment_d2(a, b, c, d))
        assert abs(got - want) <= float(cap.kappa(A, B, Cc, D)) + 64 * 2.0 ** -53, (k, got, want)
        assert abs(np.sqrt(segment_point_d2(a, b, c)) - float(cap.point_segment(A, B, Cc))) <= 64 * 2.0 ** -53, k
    a, c, d = np.array([0.1, 0.2, 0.3]), np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    assert segment_point_d2(a, a, c) == float(a @ a) and np.isclose(segment_segment_d2(a, a, c, d), 0.2 ** 2 + 0.3 ** 2) and np.isclose(segment_segment_d2(c, d, a, a), 0.2 ** 2 + 0.3 ** 2)
    assert segment_segment_d2(c, d, c + 0.5 * d, c + 0.5 * d) == 0.0


def test_evaluate_methods_against_the_simulator(make_solver):
    """ClearanceGoal, SelfClearanceGoal and TouchGoal.evaluate with capsules against bioik_eval_fitness of the host simulator on random configurations"""
    cases = cap.function_cases()
    for name in ("c19_p3_c2_obstacles_9", "c20_L3_2_O3_2", "c20_L0_1_O0_3"):
        model, group, goals = cases[name]
        t, h, pr, seed, genes = sc.setup(make_solver, model, group, goals, name, 40)
        want, _ = h.fitness(abi.FK_EXACT, seed, t.pack_params(), genes)
        g = goals[0]
        for i in range(40):
            x = pr.full(seed, genes[i:i + 1]).astype(np.float64)[0]
            f = link_transform(model, model.link_index(g.link_name()), x)
            if g.opcode == abi.GOAL_CLEARANCE:
                got = g.evaluate(f, model.collision_points(g.link_name()), model.collision_capsules(g.link_name()))
            else:
                o = g.getOtherLinkName()
                got = g.evaluate(f, link_transform(model, model.link_index(o), x), model.collision_points(g.link_name()), model.collision_points(o),
                                 model.collision_capsules(g.link_name()), model.collision_capsules(o))
            assert abs(got - want[i]) <= 1e-11 * (1 + want[i]), (name, i, got, want[i])
        assert np.any(want > 0)
        h.close()
    # existing call forms keep working
    g = ClearanceGoal(TIP, 0.01, cc.scene(3, 1))
    f = link_transform(pr2_like(), pr2_like().link_index(TIP), pr2_like().default_positions())
    pts = np.hstack(cc.spheres(3, 1)[0:1] + (cc.spheres(3, 1)[1][:, None],))
    assert g.evaluate(f, pts) == g.evaluate(f, pts, None) == g.evaluate(f, pts, np.zeros((0, 8)))
    # TouchGoal: a capsule is its two end spheres
    m = pr2_like()
    m.add_collision_box(TIP, tc.BOX)
    m.add_collision_capsules(TIP, [ROW])
    tg = TouchGoal(TIP, (0.55, -0.2, 0.7), (0.2, -0.3, 0.9))
    t, h, pr, seed, genes = sc.setup(make_solver, m, "right_arm", [tg], "touch", 20)
    want, _ = h.fitness(abi.FK_EXACT, seed, t.pack_params(), genes)
    for i in range(20):
        f = link_transform(m, m.link_index(TIP), pr.full(seed, genes[i:i + 1]).astype(np.float64)[0])
        got = tg.evaluate(f, m.collision_points(TIP), None, m.collision_capsules(TIP))
        assert abs(got - want[i]) <= 1e-12 * (1 + want[i]), (i, got, want[i])
    h.close()
