"""TouchGoal in the Python package, without a GPU: the goal class, the robot model's collision setters, the URDF reader and the host evaluation."""
import numpy as np

import touch_cases as tc
from bio_ik_amd import ProblemTemplate, TouchGoal, abi, load_urdf, pr2_like
from np_fk import LD

URDF = """<robot name="finger">
  <link name="base"/>
  <link name="pad">
    <collision><origin xyz="0.02 -0.01 0.03" rpy="0.3 -0.2 0.5"/><geometry><box size="0.10 0.06 0.04"/></geometry></collision>
    <collision><origin xyz="0.05 0.0 -0.02" rpy="0.0 0.4 0.0"/><geometry><sphere radius="0.035"/></geometry></collision>
    <collision><origin xyz="-0.01 0.02 0.0" rpy="-0.6 0.1 0.2"/><geometry><mesh filename="package://finger/pad.stl" scale="0.5 0.5 2"/></geometry></collision>
  </link>
  <link name="rod"><collision><geometry><cylinder radius="0.01" length="0.2"/></geometry></collision></link>
  <link name="plain"><collision><geometry><box size="0.2 0.4 0.6"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="pad"/><axis xyz="0 0 1"/><limit lower="-1" upper="1" velocity="1"/></joint>
  <joint name="j2" type="revolute"><parent link="pad"/><child link="rod"/><origin xyz="0.1 0 0"/><axis xyz="0 1 0"/><limit lower="-1" upper="1" velocity="1"/></joint>
  <joint name="j3" type="fixed"><parent link="rod"/><child link="plain"/></joint>
</robot>"""


def test_goal_class():
    g = TouchGoal("pad", (1, 2, 3), (0, 3, 4), weight=0.5)
    assert g.opcode == abi.GOAL_TOUCH == 17 and abi.GOAL_PARAM_COUNT[17] == 6
    assert np.array_equal(g.params(), [1, 2, 3, 0, 0.6, 0.8]) and g.getWeight() == 0.5 and not g.isSecondary() and g.link_name() == "pad"
    assert np.array_equal(g.getPosition(), [1, 2, 3]) and np.array_equal(g.getNormal(), [0, 0.6, 0.8])
    t = ProblemTemplate(tc.arm_with_box(), "right_arm", [g.__class__(tc.TIP, (1, 2, 3), (0, 0, 2))])
    assert t.param_count == 6 and np.array_equal(t.pack_params(), [1, 2, 3, 0, 0, 1])


def test_robot_setters():
    m = pr2_like()
    m.add_collision_box(tc.TIP, (0.2, 0.4, 0.6))  # an identity origin: the corners untouched
    want = [(x, y, z, 0.0) for x in (-0.1, 0.1) for y in (-0.2, 0.2) for z in (-0.3, 0.3)]
    assert np.array_equal(m.collision_points(tc.TIP), want)
    m.add_collision_sphere(tc.TIP, 0.05, (1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0))
    assert np.array_equal(m.collision_points(tc.TIP)[8], [1.0, 2.0, 3.0, 0.05])
    s = np.sqrt(0.5)
    m.add_collision_points(tc.TIP_L, [(1.0, 0.0, 0.0), (0.0, 0.0, 2.0)], [0.0, 0.25], (0.5, 0.0, 0.0, 0.0, 0.0, s, s))  # a quarter turn about z, then +0.5 x
    assert np.allclose(m.collision_points(tc.TIP_L), [(0.5, 1.0, 0.0, 0.0), (0.5, 0.0, 2.0, 0.25)], atol=1e-15, rtol=0)
    mixed = tc.mixed_model().collision_points(tc.TIP)
    assert mixed.shape == (16, 4) and np.abs(mixed - np.asarray(tc.mixed_expected(), dtype=np.float64)).max() < 8 * 2.0 ** -53
    k = tc.mixed_model().arrays()
    link = pr2_like().link_index(tc.TIP)
    assert k["link_point_first"][link] == 0 and k["link_point_first"][link + 1] == 16 and k["link_point_first"][-1] == 16
    d = pr2_like().desc()
    assert not d.link_point_first and not d.link_points  # no shapes: both NULL


def test_urdf_collisions():
    m = load_urdf(URDF)
    pad = m.collision_points("pad")
    want = np.vstack([tc.expected_box(tc.BOX, tc.O_BOX), np.hstack([tc.move([[0, 0, 0]], tc.O_SPH), [[LD(0.035)]]])])
    assert pad.shape == (9, 4) and np.abs(pad - np.asarray(want, dtype=np.float64)).max() < 8 * 2.0 ** -53
    (name, scale, origin), = m.link_meshes[m.link_index("pad")]
    assert name == "package://finger/pad.stl" and scale == (0.5, 0.5, 2.0) and np.allclose(origin[:3], (-0.01, 0.02, 0.0))
    assert np.array_equal(m.collision_points("plain"), [(x, y, z, 0.0) for x in (-0.1, 0.1) for y in (-0.2, 0.2) for z in (-0.3, 0.3)])
    assert m.collision_points("rod")[0, 3] == -1 and m.link_unsupported[m.link_index("rod")] == ["cylinder"]  # recorded as a shape without a point form
    # the pad's mesh is only named: until its vertices are supplied the pad's rows end with the marker, so a TouchGoal on it is refused, not scored on box + sphere
    k, pad_i = m.arrays(), m.link_index("pad")
    assert k["link_point_first"][pad_i + 1] - k["link_point_first"][pad_i] == 10 and k["link_points"][k["link_point_first"][pad_i + 1] - 1, 3] == -1
    m.add_collision_points("pad", tc.MESH * np.asarray(scale), None, origin)
    k = m.arrays()
    assert k["link_point_first"][pad_i + 1] - k["link_point_first"][pad_i] == 9 + len(tc.MESH) and np.all(k["link_points"][:, 3][k["link_point_first"][pad_i]:k["link_point_first"][pad_i + 1]] >= 0)
    assert len(m.collision_points("base")) == 0


def test_host_evaluation():
    rng = np.random.default_rng(4)
    pts = tc.mixed_model().collision_points(tc.TIP)
    for _ in range(50):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        f = np.concatenate([rng.uniform(-1, 1, 3), q])
        g = TouchGoal(tc.TIP, rng.uniform(-1, 1, 3), rng.normal(size=3), weight=1.0)
        d = tc.touch_distance(g.params(), f[None, :3], f[None, 3:], pts)[0]
        assert abs(g.evaluate(f, pts) - float(d * d)) <= 64 * 2.0 ** -53 * (1 + abs(float(d))) ** 2
