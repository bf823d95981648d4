"""Goal (cost) classes: host-side mirror of reference include/bio_ik/goal.h:97-129 and goal_types.h:56-712.

Same class names, constructor arguments, setters and normalisation behaviour as the reference; instead of a
virtual `evaluate` every built-in goal serialises itself into (opcode, link/variable, weight, secondary) for the
problem template and a flat parameter vector per query (`params()`), which is what the device evaluates.
Goals that need host callbacks (JointFunctionGoal, LinkFunctionGoal) have no
device opcode; constructing a problem with them raises NotImplementedError.
"""
import math

import numpy as np

from . import abi


def _vec3(v):
    a = np.asarray(v, dtype=np.float64).reshape(3)
    return a


def _normalized(v):
    a = np.asarray(v, dtype=np.float64)
    return a / math.sqrt(float(np.dot(a, a)))


class Goal:
    """reference goal.h:97-119"""
    opcode = None

    def __init__(self):
        self.weight_ = 1.0
        self.secondary_ = False

    def isSecondary(self):
        return self.secondary_

    def getWeight(self):
        return self.weight_

    def setWeight(self, w):
        self.weight_ = float(w)

    # --- serialisation hooks (the "describe-to-POD" of DESIGN.md §2) ---
    def link_name(self):
        return None

    def variable_name(self):
        return None

    def params(self):
        return np.zeros(0)


class LinkGoalBase(Goal):
    """goal_types.h:56-78"""

    def __init__(self, link_name="", weight=1.0, base_link=""):
        super().__init__()
        self.weight_ = float(weight)
        self.link_name_ = link_name
        self.base_link_name_ = base_link

    def setLinkName(self, n):
        self.link_name_ = n

    def getLinkName(self):
        return self.link_name_

    def link_name(self):
        return self.link_name_

    # BASE LINKS (include/bioik_hip.h; no reference counterpart): the goal is evaluated on the link's frame expressed in the base link's frame,
    # R = inverse(base) o link; "" (the default) is the world.  ProblemTemplate marshals it into bioik_problem_desc::goal_base_link.
    def setBaseLinkName(self, n):
        self.base_link_name_ = n

    def getBaseLinkName(self):
        return self.base_link_name_

    def base_link_name(self):
        return self.base_link_name_ or None


class PositionGoal(LinkGoalBase):
    opcode = abi.GOAL_POSITION

    def __init__(self, link_name="", position=(0, 0, 0), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.position_ = _vec3(position)

    def getPosition(self):
        return self.position_

    def setPosition(self, p):
        self.position_ = _vec3(p)

    def params(self):
        return self.position_.copy()


class OrientationGoal(LinkGoalBase):
    opcode = abi.GOAL_ORIENTATION

    def __init__(self, link_name="", orientation=(0, 0, 0, 1), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.orientation_ = _normalized(orientation)  # goal_types.h:110

    def getOrientation(self):
        return self.orientation_

    def setOrientation(self, q):
        self.orientation_ = _normalized(q)

    def params(self):
        return self.orientation_.copy()


class PoseGoal(LinkGoalBase):
    opcode = abi.GOAL_POSE

    def __init__(self, link_name="", position=(0, 0, 0), orientation=(0, 0, 0, 1), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.position_ = _vec3(position)
        self.orientation_ = _normalized(orientation)  # goal_types.h:139
        self.rotation_scale_ = 0.5                    # goal_types.h:133,140

    def getPosition(self):
        return self.position_

    def setPosition(self, p):
        self.position_ = _vec3(p)

    def getOrientation(self):
        return self.orientation_

    def setOrientation(self, q):
        self.orientation_ = _normalized(q)

    def getRotationScale(self):
        return self.rotation_scale_

    def setRotationScale(self, s):
        self.rotation_scale_ = float(s)

    def params(self):
        return np.concatenate([self.position_, self.orientation_, [self.rotation_scale_]])


class LookAtGoal(LinkGoalBase):
    opcode = abi.GOAL_LOOK_AT

    def __init__(self, link_name="", axis=(1, 0, 0), target=(0, 0, 0), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.axis_ = _vec3(axis)  # constructor does not normalise (goal_types.h:194-199); the setter does (:202)
        self.target_ = _vec3(target)

    def setAxis(self, a):
        self.axis_ = _normalized(a)

    def setTarget(self, t):
        self.target_ = _vec3(t)

    def getAxis(self):
        return self.axis_

    def getTarget(self):
        return self.target_

    def params(self):
        return np.concatenate([self.axis_, self.target_])


class _DistanceGoal(LinkGoalBase):
    def __init__(self, link_name="", target=(0, 0, 0), distance=1.0, weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.target = _vec3(target)
        self.distance = float(distance)

    def getTarget(self):
        return self.target

    def setTarget(self, t):
        self.target = _vec3(t)

    def getDistance(self):
        return self.distance

    def setDistance(self, d):
        self.distance = float(d)

    def params(self):
        return np.concatenate([self.target, [self.distance]])


class MaxDistanceGoal(_DistanceGoal):
    opcode = abi.GOAL_MAX_DISTANCE


class MinDistanceGoal(_DistanceGoal):
    opcode = abi.GOAL_MIN_DISTANCE


class LineGoal(LinkGoalBase):
    opcode = abi.GOAL_LINE

    def __init__(self, link_name="", position=(0, 0, 0), direction=(1, 0, 0), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.position = _vec3(position)
        self.direction = _normalized(direction)  # goal_types.h:286

    def setPosition(self, p):
        self.position = _vec3(p)

    def setDirection(self, d):
        self.direction = _normalized(d)

    def getPosition(self):
        return self.position

    def getDirection(self):
        return self.direction

    def params(self):
        return np.concatenate([self.position, self.direction])


class PlaneGoal(LinkGoalBase):
    opcode = abi.GOAL_PLANE

    def __init__(self, link_name="", position=(0, 0, 0), normal=(0, 0, 1), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.position = _vec3(position)
        self.normal = _normalized(normal)  # goal_types.h:314

    def setPosition(self, p):
        self.position = _vec3(p)

    def setNormal(self, n):
        self.normal = _normalized(n)

    def getPosition(self):
        return self.position

    def getNormal(self):
        return self.normal

    def params(self):
        return np.concatenate([self.position, self.normal])


_TINY = 2.2250738585072014e-308  # DBL_MIN: a segment whose squared length is not above it counts as its first end (include/bioik_hip.h: CAPSULES)


def _clamp01(x):
    return min(max(x, 0.0), 1.0)


def segment_point_d2(a, b, c):
    """CAPSULES (include/bioik_hip.h): the squared distance of the point c from the segment a b, the device's formula in float64 (unfused: equal up to rounding)"""
    u, e = b - a, c - a
    uu = float(u @ u)
    t = _clamp01(float(e @ u) * (1.0 / uu)) if uu > _TINY else 0.0
    x = e - t * u
    return float(x @ x)


def segment_segment_d2(a, b, c, d):
    """CAPSULES (include/bioik_hip.h): the squared distance of the segments a b and c d by clamped closest points, the device's formula in float64 (unfused)"""
    u, v, w = b - a, d - c, a - c
    uu, uv, vv, uw, vw = float(u @ u), float(u @ v), float(v @ v), float(u @ w), float(v @ w)
    ru = 1.0 / uu if uu > _TINY else 0.0
    rv = 1.0 / vv if vv > _TINY else 0.0
    den = uu * vv - uv * uv
    s = _clamp01((uv * vw - vv * uw) / den) if den > 0.0 else 0.0
    t = (uv * s + vw) * rv
    tc = _clamp01(t)
    if tc != t or rv == 0.0:
        s = _clamp01((uv * tc - uw) * ru)
    x = w + s * u - tc * v
    return float(x @ x)


def _rotate(q, v):  # v + 2 (w (u x v) + u x (u x v)), q as it is
    t = np.cross(q[:3], v)
    return v + 2.0 * (q[3] * t + np.cross(q[:3], t))


def _pen2(s, d2):
    return max(0.0, s - float(np.sqrt(d2))) ** 2 if s > 0 and d2 < s * s else 0.0


def _clearance_with_capsules(margin, p, q, pts, caps, obs, ocaps):
    """the part of the clearance cost that involves a capsule: the link's primitives (points, then capsules; carried over by p + rotate(q, .)) outermost, for each the
    other side's points, then its capsules (as they are); the point-against-point pairs are the caller's"""
    total = 0.0
    for v in pts:
        w = p + _rotate(q, v[:3])
        for o in ocaps:
            total += _pen2((margin + v[3]) + o[3], segment_point_d2(o[:3], o[4:7], w))
    for k in caps:
        a, b = p + _rotate(q, k[:3]), p + _rotate(q, k[4:7])
        for o in obs:
            total += _pen2((margin + k[3]) + o[3], segment_point_d2(a, b, o[:3]))
        for o in ocaps:
            total += _pen2((margin + k[3]) + o[3], segment_segment_d2(a, b, o[:3], o[4:7]))
    return total


def _rows(a, width):
    return np.zeros((0, width)) if a is None else np.asarray(a, dtype=np.float64).reshape(-1, width)


class TouchGoal(LinkGoalBase):
    """goal_types.h:330-377, goal_types.cpp:152-228: the collision shapes of the link touch the plane through `position` with `normal`.  The shapes are the
    link's collision points and disks of the robot model (RobotModel.add_collision_box / _sphere / _points / _cylinder / _cone, or the URDF reader): no FCL."""
    opcode = abi.GOAL_TOUCH

    def __init__(self, link_name="", position=(0, 0, 0), normal=(0, 0, 1), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.position = _vec3(position)
        self.normal = _normalized(normal)  # goal_types.h:371

    def getPosition(self):
        return self.position

    def getNormal(self):
        return self.normal

    def params(self):
        return np.concatenate([self.position, self.normal])

    def evaluate(self, frame, points, disks=None, capsules=None):
        """The cost on the host: frame = the link's px py pz qx qy qz qw, points [n][4] = RobotModel.collision_points(link), disks [m][8] =
        RobotModel.collision_disks(link) (optional), capsules [k][8] = RobotModel.collision_capsules(link) (optional: a capsule's support function is the smaller of
        its two end spheres', so each joins the points as A r and B r -- exact).  The device's formula in numpy."""
        f = np.asarray(frame, dtype=np.float64)
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
        for k in _rows(capsules, 8):
            pts = np.vstack([pts, [k[0], k[1], k[2], k[3]], [k[4], k[5], k[6], k[3]]])
        dks = np.zeros((0, 8)) if disks is None else np.asarray(disks, dtype=np.float64).reshape(-1, 8)
        x, y, z, w = f[3:7]
        u = np.array([-x, -y, -z])  # tf2's inverse(): the conjugate
        t = 2.0 * np.cross(u, self.normal)
        n_l = self.normal + w * t + np.cross(u, t)
        support = np.concatenate([pts[:, :3] @ n_l - pts[:, 3], dks[:, :3] @ n_l - dks[:, 3] * np.linalg.norm(np.cross(n_l[None], dks[:, 4:7]), axis=1)])
        d = float(np.min(support)) - float(np.dot(self.normal, self.position - f[:3]))
        return d * d


class ClearanceGoal(LinkGoalBase):
    """No reference counterpart (include/bioik_hip.h: BIOIK_GOAL_CLEARANCE): the spheres of the link -- the link's collision points of the robot model, each with its
    radius -- keep at least `margin` away from a table of obstacle spheres in the world frame, rows cx cy cz R, at most abi.MAX_OBSTACLES of them.  The margin is a
    per-query parameter; the table is data of the goal, shared by every query: ProblemTemplate carries it, HipSolver uploads it when the handle is created and
    HipSolver.set_obstacles replaces it on a live handle."""
    opcode = abi.GOAL_CLEARANCE

    def __init__(self, link_name="", margin=0.0, obstacles=(), weight=1.0):
        super().__init__(link_name, weight, "")
        self.margin_ = float(margin)
        self.setObstacles(obstacles)

    def getMargin(self):
        return self.margin_

    def setMargin(self, m):
        self.margin_ = float(m)

    def getObstacles(self):
        return self.obstacles_

    def setObstacles(self, spheres):
        """rows cx cy cz R: finite, R >= 0, at most abi.MAX_OBSTACLES (what bioik_problem_set_obstacles accepts)"""
        a = np.array(spheres, dtype=np.float64).reshape(-1, 4)
        if a.shape[0] > abi.MAX_OBSTACLES:
            raise ValueError("ClearanceGoal: %d obstacles, more than MAX_OBSTACLES (%d)" % (a.shape[0], abi.MAX_OBSTACLES))
        if not np.isfinite(a).all() or (a[:, 3] < 0).any():
            raise ValueError("ClearanceGoal: an obstacle row must be finite with a radius >= 0")
        self.obstacles_ = np.ascontiguousarray(a)

    def params(self):
        return np.array([self.margin_])

    def evaluate(self, frame, points, capsules=None):
        """The cost on the host: frame = the link's px py pz qx qy qz qw, points [n][4] = RobotModel.collision_points(link), capsules [k][8] =
        RobotModel.collision_capsules(link) (optional).  The device's formula in numpy (plain multiplications and additions where the device fuses them: equal up
        to rounding): the points against every obstacle, then the capsules against every obstacle."""
        f = np.asarray(frame, dtype=np.float64)
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
        caps = _rows(capsules, 8)
        obs = self.obstacles_
        if obs.shape[0] == 0 or pts.shape[0] + caps.shape[0] == 0:
            return 0.0
        total = 0.0
        if pts.shape[0]:
            u, w = f[3:6], f[6]
            t = np.cross(u[None], pts[:, :3])
            world = f[None, :3] + pts[:, :3] + 2.0 * (w * t + np.cross(u[None], t))  # q as it is, not normalised
            s = (self.margin_ + pts[:, 3])[:, None] + obs[None, :, 3]
            d = np.linalg.norm(world[:, None, :] - obs[None, :, :3], axis=2)
            pen = np.where(s > 0, np.maximum(0.0, s - d), 0.0)
            total = float((pen * pen).sum())
        return total + _clearance_with_capsules(self.margin_, f[:3], f[3:], np.zeros((0, 4)), caps, obs, np.zeros((0, 8)))


class SelfClearanceGoal(LinkGoalBase):
    """No reference counterpart (include/bioik_hip.h: BIOIK_GOAL_SELF_CLEARANCE): the spheres of the link -- its collision points of the robot model, each with its
    radius -- keep at least `margin` away from the spheres of ANOTHER link of the same robot.  The other link is the goal's base link (BASE LINKS): the cost is
    ClearanceGoal's, read in the other link's frame R = inverse(other) o link, with the other link's points as the obstacle table.  Both tables are the model's: the
    goal carries the two names and the margin (a per-query parameter)."""
    opcode = abi.GOAL_SELF_CLEARANCE

    def __init__(self, link_name="", other_link="", margin=0.0, weight=1.0):
        super().__init__(link_name, weight, other_link)
        self.margin_ = float(margin)

    def getMargin(self):
        return self.margin_

    def setMargin(self, m):
        self.margin_ = float(m)

    def setOtherLinkName(self, n):
        self.setBaseLinkName(n)

    def getOtherLinkName(self):
        return self.getBaseLinkName()

    def params(self):
        return np.array([self.margin_])

    def evaluate(self, frame, other_frame, points, other_points, capsules=None, other_capsules=None):
        """The cost on the host: frame / other_frame = the link's and the other link's px py pz qx qy qz qw, points [n][4] / other_points [m][4] =
        RobotModel.collision_points of the two, capsules [k][8] / other_capsules [k'][8] = RobotModel.collision_capsules of the two (optional).  The device's formula
        in numpy (plain multiplications and additions where the device fuses them: equal up to rounding); quaternions as they are, not normalised."""
        b, a = np.asarray(frame, dtype=np.float64), np.asarray(other_frame, dtype=np.float64)
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
        obs = np.asarray(other_points, dtype=np.float64).reshape(-1, 4)
        caps, ocaps = _rows(capsules, 8), _rows(other_capsules, 8)
        if obs.shape[0] + ocaps.shape[0] == 0 or pts.shape[0] + caps.shape[0] == 0:
            return 0.0

        def mul(p, q):
            return np.append(p[3] * q[:3] + q[3] * p[:3] + np.cross(p[:3], q[:3]), p[3] * q[3] - p[:3] @ q[:3])
        c = a[3:] * np.array([-1.0, -1.0, -1.0, 1.0])  # R = concat(invert(A), B)
        rp, rq = _rotate(c, -a[:3]) + _rotate(c, b[:3]), mul(c, b[3:])
        total = 0.0
        if pts.shape[0] and obs.shape[0]:
            centres = rp[None] + np.array([_rotate(rq, v) for v in pts[:, :3]])
            s = (self.margin_ + pts[:, 3])[:, None] + obs[None, :, 3]
            d = np.linalg.norm(centres[:, None, :] - obs[None, :, :3], axis=2)
            pen = np.where(s > 0, np.maximum(0.0, s - d), 0.0)
            total = float((pen * pen).sum())
        return total + _clearance_with_capsules(self.margin_, rp, rq, pts, caps, obs, ocaps)


class _JointSetGoal(Goal):
    def __init__(self, weight=1.0, secondary=True):
        super().__init__()
        self.weight_ = float(weight)
        self.secondary_ = bool(secondary)


class AvoidJointLimitsGoal(_JointSetGoal):
    opcode = abi.GOAL_AVOID_JOINT_LIMITS


class CenterJointsGoal(_JointSetGoal):
    opcode = abi.GOAL_CENTER_JOINTS


class MinimalDisplacementGoal(_JointSetGoal):
    opcode = abi.GOAL_MINIMAL_DISPLACEMENT


class RegularizationGoal(Goal):
    opcode = abi.GOAL_REGULARIZATION

    def __init__(self, weight=1.0):
        super().__init__()
        self.weight_ = float(weight)


class JointVariableGoal(Goal):
    opcode = abi.GOAL_JOINT_VARIABLE

    def __init__(self, variable_name="", variable_position=0.0, weight=1.0, secondary=False):
        super().__init__()
        self.variable_name_ = variable_name
        self.variable_position = float(variable_position)
        self.weight_ = float(weight)
        self.secondary_ = bool(secondary)

    def getVariablePosition(self):
        return self.variable_position

    def setVariablePosition(self, p):
        self.variable_position = float(p)

    def getVariableName(self):
        return self.variable_name_

    def setVariableName(self, n):
        self.variable_name_ = n

    def variable_name(self):
        return self.variable_name_

    def params(self):
        return np.array([self.variable_position])


class _AxisDirectionGoal(LinkGoalBase):
    def __init__(self, link_name="", axis=(0, 0, 1), direction=(0, 0, 1), weight=1.0, base_link=""):
        super().__init__(link_name, weight, base_link)
        self.axis = _vec3(axis)  # constructors do not normalise (goal_types.h:596-601, 627-632); setters do
        self.direction = _vec3(direction)

    def setAxis(self, a):
        self.axis = _normalized(a)

    def setDirection(self, d):
        self.direction = _normalized(d)

    def getAxis(self):
        return self.axis

    def getDirection(self):
        return self.direction

    def params(self):
        return np.concatenate([self.axis, self.direction])


class SideGoal(_AxisDirectionGoal):
    opcode = abi.GOAL_SIDE


class DirectionGoal(_AxisDirectionGoal):
    opcode = abi.GOAL_DIRECTION


class ConeGoal(LinkGoalBase):
    opcode = abi.GOAL_CONE

    def __init__(self, link_name="", axis=(0, 0, 1), direction=(0, 0, 1), angle=0.0, weight=1.0, position=None,
                 position_weight=None, base_link=""):
        super().__init__(link_name, weight, base_link)
        # three reference constructors, goal_types.h:673-699
        self.position = _vec3(position if position is not None else (0, 0, 0))
        self.position_weight = float(position_weight if position_weight is not None else (1.0 if position is not None else 0.0))
        self.axis = _vec3(axis)
        self.direction = _vec3(direction)
        self.angle = float(angle)

    def setPosition(self, p):
        self.position = _vec3(p)

    def setPositionWeight(self, w):
        self.position_weight = float(w)

    def setAxis(self, a):
        self.axis = _normalized(a)

    def setDirection(self, d):
        self.direction = _normalized(d)

    def setAngle(self, a):
        self.angle = float(a)

    def params(self):
        return np.concatenate([self.position, [self.position_weight], self.axis, self.direction, [self.angle]])


class BalanceGoal(Goal):
    """goal_types.h:540-566, goal_types.cpp:231-272: keeps the centre of mass of the whole robot (every link with a URDF <inertial>)
    over `target`, measured perpendicular to `axis` (the direction of gravity).  The link masses are part of the robot model
    (RobotModel.add_link(mass=, com=) / the URDF reader); every link with mass becomes a tip of the problem."""
    opcode = abi.GOAL_BALANCE

    def __init__(self, target=(0, 0, 0), weight=1.0):
        super().__init__()
        self.target = _vec3(target)
        self.axis = _vec3((0, 0, 1))
        self.weight_ = float(weight)

    def getTarget(self):
        return self.target

    def getAxis(self):
        return self.axis

    def setTarget(self, t):
        self.target = _vec3(t)

    def setAxis(self, a):
        self.axis = _vec3(a)  # (the reference's setter does not normalise, goal_types.h:562)

    def params(self):
        return np.concatenate([self.target, self.axis])


class _HostOnlyGoal(Goal):
    """Goals evaluated through arbitrary host code in the reference: no device opcode."""
    opcode = None


class JointFunctionGoal(_HostOnlyGoal):
    def __init__(self, variable_names=(), function=None, weight=1.0, secondary=False):
        super().__init__()
        self.variable_names = list(variable_names)
        self.function = function
        self.weight_ = float(weight)
        self.secondary_ = bool(secondary)


class LinkFunctionGoal(_HostOnlyGoal):
    def __init__(self, link_name="", function=None, weight=1.0):
        super().__init__()
        self.link_name_ = link_name
        self.function = function
        self.weight_ = float(weight)


class BioIKKinematicsQueryOptions:
    """reference goal.h:121-129 (kinematics::KinematicsQueryOptions fields included)."""

    def __init__(self):
        self.goals = []
        self.fixed_joints = []
        self.replace = False
        self.solution_fitness = 0.0
        self.return_approximate_solution = False
