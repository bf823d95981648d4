"""Cylinders and cones for TouchGoal in the Python package, without a GPU: the long-double restatement of the disk term (tests/touch_disk_cases.py) against
the brute-force minimum over points sampled on the rim, the robot model's setters, the URDF reader's recorded solids and the host evaluation."""
import numpy as np
import pytest

import touch_cases as tc
import touch_disk_cases as td
from bio_ik_amd import ProblemTemplate, TouchGoal, abi, load_urdf, pr2_like
from bio_ik_amd.robot import quat_from_rpy
from np_fk import LD
from test_touch_goal_api import URDF


def rim_points(disk, n):
    """n points on the rim of a disk cx cy cz r ax ay az: long double, by two unit vectors orthogonal to the axis (not by the closed form)"""
    c, r, a = np.asarray(disk[:3], dtype=LD), LD(disk[3]), np.asarray(disk[4:7], dtype=LD)
    e = np.zeros(3, dtype=LD)
    e[int(np.argmin(np.abs(a)))] = 1
    u = np.cross(a, e)
    u /= np.sqrt(u @ u)
    w = np.cross(a, u)
    w /= np.sqrt(w @ w)
    phi = 2 * LD(np.pi) * np.arange(n, dtype=LD) / n
    return c[None] + r * (np.cos(phi)[:, None] * u[None] + np.sin(phi)[:, None] * w[None])


def test_restatement_against_sampled_rims():
    """The closed form n . c - r |n x a| is the minimum of n . x over the rim: the minimum over N rim points is never below it, and above it by no more than
    r |n x a| (1 - cos(pi / N)) <= r (1 - cos(pi / N)) -- the lowest rim point is at most half a step pi / N away from a sampled one.  Geometry, not a tolerance:
    the slack is 64 roundings of the long-double sums."""
    rng = np.random.default_rng(12)
    N = 360
    tiny = 64 * float(np.finfo(LD).eps)
    disks = td.random_disks(40, 5, scale=0.5, rmax=0.3)
    normals = rng.normal(size=(40, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    cases = [(k, n) for k in disks for n in normals[:8]]
    for k in disks[:8]:  # exactly parallel and exactly perpendicular to the axis (an axis along z, so that both are exact in doubles)
        kz = np.concatenate([k[:4], [0.0, 0.0, 1.0]])
        cases += [(kz, np.array([0.0, 0.0, 1.0])), (kz, np.array([0.0, 0.0, -1.0])), (kz, np.array([1.0, 0.0, 0.0])), (kz, np.array([0.6, -0.8, 0.0]))]
    for k, n in cases:
        closed = td.disk_support(np.asarray(n, dtype=LD)[None], np.concatenate([k, [0.0]])[None])[0, 0]
        sampled = (rim_points(k, N) @ np.asarray(n, dtype=LD)).min()
        scale = tiny * (1 + np.linalg.norm(k[:3]) + k[3])
        assert sampled >= closed - scale, (k, n, float(sampled - closed))
        assert sampled - closed <= LD(k[3]) * (1 - np.cos(LD(np.pi) / N)) + scale, (k, n, float(sampled - closed))
    kz = np.array([0.1, 0.2, 0.3, 0.25, 0.0, 0.0, 1.0, 0.0])
    assert td.disk_support(np.array([[0, 0, 1]], dtype=LD), kz[None])[0, 0] == LD(0.3)  # parallel: no radius in it
    assert td.disk_support(np.array([[1, 0, 0]], dtype=LD), kz[None])[0, 0] == LD(0.1) - LD(0.25)  # perpendicular: the whole radius


def test_robot_setters():
    m = pr2_like()
    m.add_collision_cylinder(tc.TIP, 0.03, 0.2)  # an identity origin: the rows untouched
    assert np.array_equal(m.collision_disks(tc.TIP), [(0, 0, -0.1, 0.03, 0, 0, 1, 0), (0, 0, 0.1, 0.03, 0, 0, 1, 0)]) and len(m.collision_points(tc.TIP)) == 0
    m.add_collision_cone(tc.TIP_L, 0.04, 0.1, td.IDENT)  # MoveIt's shapes::Cone: the origin halfway up, the tip on +z
    assert np.array_equal(m.collision_disks(tc.TIP_L), [(0, 0, -0.05, 0.04, 0, 0, 1, 0)]) and np.array_equal(m.collision_points(tc.TIP_L), [(0, 0, 0.05, 0)])
    # a rotated origin: a quarter turn about x (z -> -y), then the shift
    s = np.sqrt(0.5)
    o = (0.5, 0.0, -0.25, s, 0.0, 0.0, s)
    r = pr2_like()
    r.add_collision_cylinder(tc.TIP, 0.03, 0.2, o)
    r.add_collision_cone(tc.TIP_L, 0.04, 0.1, o)
    assert np.allclose(r.collision_disks(tc.TIP), [(0.5, 0.1, -0.25, 0.03, 0, -1, 0, 0), (0.5, -0.1, -0.25, 0.03, 0, -1, 0, 0)], atol=4e-16, rtol=0)
    assert np.allclose(r.collision_disks(tc.TIP_L), [(0.5, 0.05, -0.25, 0.04, 0, -1, 0, 0)], atol=4e-16, rtol=0)
    assert np.allclose(r.collision_points(tc.TIP_L), [(0.5, -0.05, -0.25, 0)], atol=4e-16, rtol=0)
    # ... and a general one, against the rotation matrix of its rpy in long double
    rpy, xyz = (0.3, -0.2, 0.5), (0.02, -0.01, 0.03)
    g = pr2_like()
    g.add_collision_cylinder(tc.TIP, 0.03, 0.2, xyz + tuple(quat_from_rpy(*rpy)))
    want_c = tc.move([[0, 0, -0.1], [0, 0, 0.1]], (xyz, rpy))
    want_a = tc.move([[0, 0, 1]], ((0, 0, 0), rpy))
    got = g.collision_disks(tc.TIP)
    assert np.abs(got[:, :3] - np.asarray(want_c, dtype=np.float64)).max() < 8 * 2.0 ** -53 and np.abs(got[:, 4:7] - np.asarray(want_a, dtype=np.float64)).max() < 8 * 2.0 ** -53
    assert np.array_equal(got[:, 3], [0.03, 0.03]) and np.array_equal(got[:, 7], [0, 0])
    # raw rows, and what they refuse
    m.add_collision_disks(tc.TIP, [(1, 2, 3, 0.5, 0, 0.6, 0.8)])
    assert np.array_equal(m.collision_disks(tc.TIP)[2], (1, 2, 3, 0.5, 0, 0.6, 0.8, 0))
    for bad in ((0, 0, 0, -0.1, 0, 0, 1), (0, 0, 0, 0.1, 0, 0, 1.1), (0, 0, np.nan, 0.1, 0, 0, 1)):
        with pytest.raises(ValueError):
            m.add_collision_disks(tc.TIP, [bad])
    # arrays(): the offsets of the pair; desc(): NULL without disks
    k = m.arrays()
    tip, tip_l = m.link_index(tc.TIP), m.link_index(tc.TIP_L)
    first = k["link_disk_first"]
    assert first.dtype == np.int32 and len(first) == m.n_links + 1 and first[0] == 0 and first[-1] == 4 and k["link_disks"].shape == (4, 8)
    assert first[tip + 1] - first[tip] == 3 and first[tip_l + 1] - first[tip_l] == 1 and np.all(np.diff(first) >= 0)
    assert np.array_equal(k["link_disks"][first[tip]:first[tip + 1]], m.collision_disks(tc.TIP))
    d = m.desc()
    assert d.link_disk_first and d.link_disks and d.link_point_first and d.struct_size == abi.C.sizeof(abi.ModelDesc)
    d = tc.arm_with_box().desc()
    assert not d.link_disk_first and not d.link_disks and d.link_point_first
    d = pr2_like().desc()
    assert not d.link_disk_first and not d.link_disks and not d.link_point_first


def test_urdf_solids_are_resolved_on_request():
    m = load_urdf(URDF)
    rod = m.link_index("rod")
    # as the reader leaves it (pinned by tests/test_touch_goal_api.py): the marker row, refused
    assert m.collision_points("rod")[0, 3] == -1 and m.link_unsupported[rod] == ["cylinder"] and len(m.collision_disks("rod")) == 0
    (kind, radius, length, origin), = m.link_solids[rod]
    assert (kind, radius, length) == ("cylinder", 0.01, 0.2) and tuple(origin) == td.IDENT
    pad_before = m.collision_points("pad").copy()
    m.resolve_collision_solids("rod")
    assert np.array_equal(m.collision_disks("rod"), [(0, 0, -0.1, 0.01, 0, 0, 1, 0), (0, 0, 0.1, 0.01, 0, 0, 1, 0)])
    assert len(m.collision_points("rod")) == 0 and m.link_unsupported.get(rod, []) == [] and rod not in m.link_solids
    k = m.arrays()
    assert k["link_point_first"][rod + 1] == k["link_point_first"][rod] and k["link_disk_first"][rod + 1] - k["link_disk_first"][rod] == 2
    assert np.array_equal(m.collision_points("pad"), pad_before)  # (nothing else moved)
    m.resolve_collision_solids()  # nothing left: no change
    assert len(m.collision_disks("rod")) == 2
    # a marker the caller set stays: only the solids' own markers go
    m2 = load_urdf(URDF)
    m2.add_collision_unsupported("rod", "cone")
    m2.resolve_collision_solids()
    assert m2.link_unsupported[rod] == ["cone"] and np.array_equal(m2.collision_points("rod"), [(0, 0, 0, -1)]) and len(m2.collision_disks("rod")) == 2
    # a collision origin on the cylinder is applied
    m3 = load_urdf(URDF.replace('<link name="rod"><collision>', '<link name="rod"><collision><origin xyz="0.1 0 0" rpy="1.5707963267948966 0 0"/>'))
    m3.resolve_collision_solids()
    assert np.allclose(m3.collision_disks("rod"), [(0.1, 0.1, 0, 0.01, 0, -1, 0, 0), (0.1, -0.1, 0, 0.01, 0, -1, 0, 0)], atol=1e-15, rtol=0)


def test_host_evaluation():
    rng = np.random.default_rng(4)
    m = td.function_cases()["two_links"][0]
    pts, dks = m.collision_points(tc.TIP), m.collision_disks(tc.TIP)
    assert len(pts) == 8 and len(dks) == 2
    for it in range(60):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        f = np.concatenate([rng.uniform(-1, 1, 3), q])
        g = TouchGoal(tc.TIP, rng.uniform(-1, 1, 3), rng.normal(size=3), weight=1.0)
        use_pts = pts if it % 3 else pts[:0]  # (disks only, too)
        d = td.touch_distance(g.params(), f[None, :3], f[None, 3:], use_pts, dks)[0]
        assert abs(g.evaluate(f, use_pts, dks) - float(d * d)) <= 64 * 2.0 ** -53 * (1 + abs(float(d))) ** 2
    d = td.touch_distance(g.params(), f[None, :3], f[None, 3:], pts, dks[:0])[0]  # without the argument: the points alone, as before
    assert abs(g.evaluate(f, pts) - float(d * d)) <= 64 * 2.0 ** -53 * (1 + abs(float(d))) ** 2
    t = ProblemTemplate(td.arm_with_cylinder(), "right_arm", [TouchGoal(tc.TIP)])
    assert t.param_count == 6
