// bio_ik/goal_types.h — the reference's built-in goal classes (include/bio_ik/goal_types.h:56-712) with the same names,
// constructors, setters, normalisation behaviour, `describe()` and `evaluate()`.  `evaluate()` is the closed form of the cost as the
// reference defines it (the solver kernels evaluate the same expression for a whole population, bio_ik_amd/csrc/bioik_device.h:
// goal_eval; tests/cpp hold one against the other); the gpu*() members serialise the goal for the device (bio_ik/goal.h).
#pragma once
#include <functional>

#include "goal.h"

namespace bio_ik {

class LinkGoalBase : public Goal {  // goal_types.h:56-78
    std::string link_name_;
    std::string base_link_name_;  // BASE LINKS (include/bioik_hip.h; no reference counterpart): "" = the world

public:
    LinkGoalBase() { weight_ = 1; }
    LinkGoalBase(const std::string& link_name, double weight) : link_name_(link_name) { weight_ = weight; }
    void setLinkName(const std::string& n) { link_name_ = n; }
    const std::string& getLinkName() const { return link_name_; }
    // A built-in link goal with a base link is evaluated on its link's frame expressed in the base link's, R = concat(inverse(base), link): what a
    // reference user writes as a Goal subclass with two addLink calls and a relative transform in evaluate()
    void setBaseLinkName(const std::string& n) { base_link_name_ = n; }
    const std::string& getBaseLinkName() const { return base_link_name_; }
    void describe(GoalContext& context) const override {
        Goal::describe(context);
        context.addLink(link_name_);
        if (!base_link_name_.empty()) context.addLink(base_link_name_);  // behind the goal's own link: getLinkFrame(1)
    }
    std::string gpuLinkName() const override { return link_name_; }
    std::string gpuBaseLinkName() const override { return base_link_name_; }

protected:
    // the frame the built-in goals read: the link's, or R for a goal with a base link (the device's formula, bioik_device.h: based_frame)
    Frame goalFrame(const GoalContext& context) const {
        return base_link_name_.empty() ? context.getLinkFrame() : concat(inverse(context.getLinkFrame(1)), context.getLinkFrame(0));
    }
};

class PositionGoal : public LinkGoalBase {  // :80-97
    Vector3 position_;

public:
    PositionGoal() : position_(0, 0, 0) {}
    PositionGoal(const std::string& link_name, const Vector3& position, double weight = 1.0) : LinkGoalBase(link_name, weight), position_(position) {}
    const Vector3& getPosition() const { return position_; }
    void setPosition(const Vector3& p) { position_ = p; }
    double evaluate(const GoalContext& context) const override { return goalFrame(context).getPosition().distance2(getPosition()); }
    int gpuOpcode() const override { return BIOIK_GOAL_POSITION; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {position_.x(), position_.y(), position_.z()}); }
};

// the orientation cost of the reference: squared distance of the two quaternions, q and -q being the same rotation (:115-124)
inline double quaternionDistance2(const Quaternion& goal, const Quaternion& q) { return std::fmin((goal - q).length2(), (goal + q).length2()); }

class OrientationGoal : public LinkGoalBase {  // :99-124
    Quaternion orientation_;

public:
    OrientationGoal() : orientation_(0, 0, 0, 1) {}
    OrientationGoal(const std::string& link_name, const Quaternion& orientation, double weight = 1.0)
        : LinkGoalBase(link_name, weight), orientation_(orientation.normalized()) {}
    const Quaternion& getOrientation() const { return orientation_; }
    void setOrientation(const Quaternion& q) { orientation_ = q.normalized(); }
    double evaluate(const GoalContext& context) const override { return quaternionDistance2(getOrientation(), goalFrame(context).getOrientation()); }
    int gpuOpcode() const override { return BIOIK_GOAL_ORIENTATION; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {orientation_.x(), orientation_.y(), orientation_.z(), orientation_.w()}); }
};

class PoseGoal : public LinkGoalBase {  // :126-181
    Vector3 position_;
    Quaternion orientation_;
    double rotation_scale_ = 0.5;

public:
    PoseGoal() : position_(0, 0, 0), orientation_(0, 0, 0, 1) {}
    PoseGoal(const std::string& link_name, const Vector3& position, const Quaternion& orientation, double weight = 1.0)
        : LinkGoalBase(link_name, weight), position_(position), orientation_(orientation.normalized()) {}
    const Vector3& getPosition() const { return position_; }
    void setPosition(const Vector3& p) { position_ = p; }
    const Quaternion& getOrientation() const { return orientation_; }
    void setOrientation(const Quaternion& q) { orientation_ = q.normalized(); }
    double getRotationScale() const { return rotation_scale_; }
    void setRotationScale(double s) { rotation_scale_ = s; }
    double evaluate(const GoalContext& context) const override {
        const Frame f = goalFrame(context);
        return f.getPosition().distance2(getPosition()) + quaternionDistance2(getOrientation(), f.getOrientation()) * (rotation_scale_ * rotation_scale_);
    }
    int gpuOpcode() const override { return BIOIK_GOAL_POSE; }
    void gpuParams(std::vector<double>& o) const override {
        o.insert(o.end(), {position_.x(), position_.y(), position_.z(), orientation_.x(), orientation_.y(), orientation_.z(), orientation_.w(), rotation_scale_});
    }
};

class LookAtGoal : public LinkGoalBase {  // :183-212
    Vector3 axis_, target_;

public:
    LookAtGoal() : axis_(1, 0, 0), target_(0, 0, 0) {}
    LookAtGoal(const std::string& link_name, const Vector3& axis, const Vector3& target, double weight = 1.0)
        : LinkGoalBase(link_name, weight), axis_(axis), target_(target) {}
    const Vector3& getAxis() const { return axis_; }
    const Vector3& getTarget() const { return target_; }
    void setAxis(const Vector3& a) { axis_ = a.normalized(); }
    void setTarget(const Vector3& t) { target_ = t; }
    double evaluate(const GoalContext& context) const override {
        const Frame f = goalFrame(context);
        const Vector3 axis = quatRotate(f.getOrientation(), axis_);
        return (target_ - f.getPosition()).normalized().distance2(axis.normalized());
    }
    int gpuOpcode() const override { return BIOIK_GOAL_LOOK_AT; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {axis_.x(), axis_.y(), axis_.z(), target_.x(), target_.y(), target_.z()}); }
};

class MaxDistanceGoal : public LinkGoalBase {  // :214-241
protected:
    Vector3 target;
    double distance = 1;

public:
    MaxDistanceGoal() : target(0, 0, 0) {}
    MaxDistanceGoal(const std::string& link_name, const Vector3& target_, double distance_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), target(target_), distance(distance_) {}
    const Vector3& getTarget() const { return target; }
    void setTarget(const Vector3& t) { target = t; }
    double getDistance() const { return distance; }
    void setDistance(double d) { distance = d; }
    double evaluate(const GoalContext& context) const override {
        const double d = std::fmax(0.0, goalFrame(context).getPosition().distance(target) - distance);
        return d * d;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_MAX_DISTANCE; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {target.x(), target.y(), target.z(), distance}); }
};

class MinDistanceGoal : public MaxDistanceGoal {  // :243-270
public:
    using MaxDistanceGoal::MaxDistanceGoal;
    double evaluate(const GoalContext& context) const override {
        const double d = std::fmax(0.0, distance - goalFrame(context).getPosition().distance(target));
        return d * d;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_MIN_DISTANCE; }
};

class LineGoal : public LinkGoalBase {  // :272-298
    Vector3 position, direction;

public:
    LineGoal() : position(0, 0, 0), direction(1, 0, 0) {}
    LineGoal(const std::string& link_name, const Vector3& position_, const Vector3& direction_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), position(position_), direction(direction_.normalized()) {}
    const Vector3& getPosition() const { return position; }
    void setPosition(const Vector3& p) { position = p; }
    const Vector3& getDirection() const { return direction; }
    void setDirection(const Vector3& d) { direction = d.normalized(); }
    double evaluate(const GoalContext& context) const override {
        const Vector3 p = goalFrame(context).getPosition();
        return position.distance2(p - direction * direction.dot(p - position));
    }
    int gpuOpcode() const override { return BIOIK_GOAL_LINE; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {position.x(), position.y(), position.z(), direction.x(), direction.y(), direction.z()}); }
};

class PlaneGoal : public LinkGoalBase {  // :300-328
    Vector3 position, normal;

public:
    PlaneGoal() : position(0, 0, 0), normal(0, 0, 1) {}
    PlaneGoal(const std::string& link_name, const Vector3& position_, const Vector3& normal_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), position(position_), normal(normal_.normalized()) {}
    const Vector3& getPosition() const { return position; }
    void setPosition(const Vector3& p) { position = p; }
    const Vector3& getNormal() const { return normal; }
    void setNormal(const Vector3& n) { normal = n.normalized(); }
    double evaluate(const GoalContext& context) const override {
        const double d = (goalFrame(context).getPosition() - position).dot(normal);
        return d * d;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_PLANE; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {position.x(), position.y(), position.z(), normal.x(), normal.y(), normal.z()}); }
};

// ---- goals over the joint values (:379-499) -------------------------------------------------------------------------------------
class AvoidJointLimitsGoal : public Goal {  // :379-402
public:
    AvoidJointLimitsGoal(double weight = 1.0, bool secondary = true) {
        weight_ = weight;
        secondary_ = secondary;
    }
    double evaluate(const GoalContext& context) const override {
        const RobotInfo& info = context.getRobotInfo();
        double sum = 0.0;
        for (size_t i = 0; i < context.getProblemVariableCount(); i++) {
            const size_t ivar = context.getProblemVariableIndex(i);
            if (info.getClipMax(ivar) == DBL_MAX) continue;
            double d = context.getProblemVariablePosition(i) - (info.getMin(ivar) + info.getMax(ivar)) * 0.5;
            d = std::fmax(0.0, std::fabs(d) * 2.0 - info.getSpan(ivar) * 0.5);
            d *= context.getProblemVariableWeight(i);
            sum += d * d;
        }
        return sum;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_AVOID_JOINT_LIMITS; }
};
class CenterJointsGoal : public Goal {  // :404-426
public:
    CenterJointsGoal(double weight = 1.0, bool secondary = true) {
        weight_ = weight;
        secondary_ = secondary;
    }
    double evaluate(const GoalContext& context) const override {
        const RobotInfo& info = context.getRobotInfo();
        double sum = 0.0;
        for (size_t i = 0; i < context.getProblemVariableCount(); i++) {
            const size_t ivar = context.getProblemVariableIndex(i);
            if (info.getClipMax(ivar) == DBL_MAX) continue;
            double d = context.getProblemVariablePosition(i) - (info.getMin(ivar) + info.getMax(ivar)) * 0.5;
            d *= context.getProblemVariableWeight(i);
            sum += d * d;
        }
        return sum;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_CENTER_JOINTS; }
};
class RegularizationGoal : public Goal {  // :428-445
public:
    RegularizationGoal(double weight = 1.0) { weight_ = weight; }
    double evaluate(const GoalContext& context) const override {
        double sum = 0.0;
        for (size_t i = 0; i < context.getProblemVariableCount(); i++) {
            const double d = context.getProblemVariablePosition(i) - context.getProblemVariableInitialGuess(i);
            sum += d * d;
        }
        return sum;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_REGULARIZATION; }
};
class MinimalDisplacementGoal : public Goal {  // :447-466
public:
    MinimalDisplacementGoal(double weight = 1.0, bool secondary = true) {
        weight_ = weight;
        secondary_ = secondary;
    }
    double evaluate(const GoalContext& context) const override {
        double sum = 0.0;
        for (size_t i = 0; i < context.getProblemVariableCount(); i++) {
            double d = context.getProblemVariablePosition(i) - context.getProblemVariableInitialGuess(i);
            d *= context.getProblemVariableWeight(i);
            sum += d * d;
        }
        return sum;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_MINIMAL_DISPLACEMENT; }
};

class JointVariableGoal : public Goal {  // :468-499
    std::string variable_name;
    double variable_position = 0;

public:
    JointVariableGoal() {}
    JointVariableGoal(const std::string& variable_name_, double variable_position_, double weight = 1.0, bool secondary = false)
        : variable_name(variable_name_), variable_position(variable_position_) {
        weight_ = weight;
        secondary_ = secondary;
    }
    double getVariablePosition() const { return variable_position; }
    void setVariablePosition(double p) { variable_position = p; }
    const std::string& getVariableName() const { return variable_name; }
    void setVariableName(const std::string& n) { variable_name = n; }
    void describe(GoalContext& context) const override {
        Goal::describe(context);
        context.addVariable(variable_name);
    }
    double evaluate(const GoalContext& context) const override {
        const double d = variable_position - context.getVariablePosition();
        return d * d;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_JOINT_VARIABLE; }
    std::string gpuVariableName() const override { return variable_name; }
    void gpuParams(std::vector<double>& o) const override { o.push_back(variable_position); }
};

// ---- host-callback goals (:501-583): any function of the joint values / of a link frame.  No device opcode: they are evaluated on
//      the host (bio_ik/goal_eval.h) and cannot be part of a device solve (the plugin refuses them with a message). ----------------
class JointFunctionGoal : public Goal {  // :501-538
    std::vector<std::string> variable_names;
    std::function<void(std::vector<double>&)> function;

public:
    JointFunctionGoal() {}
    JointFunctionGoal(const std::vector<std::string>& variable_names_, const std::function<void(std::vector<double>&)>& function_, double weight = 1.0,
                      bool secondary = false)
        : variable_names(variable_names_), function(function_) {
        weight_ = weight;
        secondary_ = secondary;
    }
    void setJointVariableNames(const std::vector<std::string>& n) { variable_names = n; }
    void setJointVariableFunction(const std::function<void(std::vector<double>&)>& f) { function = f; }
    void describe(GoalContext& context) const override {
        Goal::describe(context);
        for (auto& name : variable_names) context.addVariable(name);
    }
    double evaluate(const GoalContext& context) const override {  // squared distance between the values and what the function makes of them
        std::vector<double>& temp = context.getTempVector();
        temp.resize(variable_names.size());
        for (size_t i = 0; i < variable_names.size(); i++) temp[i] = context.getVariablePosition(i);
        function(temp);
        double sum = 0.0;
        for (size_t i = 0; i < variable_names.size(); i++) {
            const double d = temp[i] - context.getVariablePosition(i);
            sum += d * d;
        }
        return sum;
    }
};
class LinkFunctionGoal : public LinkGoalBase {  // :570-583
    std::function<double(const Vector3&, const Quaternion&)> function;

public:
    LinkFunctionGoal() {}
    LinkFunctionGoal(const std::string& link_name, const std::function<double(const Vector3&, const Quaternion&)>& function_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), function(function_) {}
    void setLinkFunction(const std::function<double(const Vector3&, const Quaternion&)>& f) { function = f; }
    double evaluate(const GoalContext& context) const override { return function(context.getLinkFrame().getPosition(), context.getLinkFrame().getOrientation()); }
};

// ---- direction goals (:585-712) -------------------------------------------------------------------------------------------------
class SideGoal : public LinkGoalBase {  // :585-614 (constructors do not normalise, setters do)
protected:
    Vector3 axis, direction;

public:
    SideGoal() : axis(0, 0, 1), direction(0, 0, 1) {}
    SideGoal(const std::string& link_name, const Vector3& axis_, const Vector3& direction_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), axis(axis_), direction(direction_) {}
    const Vector3& getAxis() const { return axis; }
    const Vector3& getDirection() const { return direction; }
    void setAxis(const Vector3& a) { axis = a.normalized(); }
    void setDirection(const Vector3& d) { direction = d.normalized(); }
    double evaluate(const GoalContext& context) const override {
        const double f = std::fmax(0.0, quatRotate(goalFrame(context).getOrientation(), axis).dot(direction));
        return f * f;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_SIDE; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {axis.x(), axis.y(), axis.z(), direction.x(), direction.y(), direction.z()}); }
};
class DirectionGoal : public SideGoal {  // :616-644
public:
    using SideGoal::SideGoal;
    double evaluate(const GoalContext& context) const override { return quatRotate(goalFrame(context).getOrientation(), axis).distance2(direction); }
    int gpuOpcode() const override { return BIOIK_GOAL_DIRECTION; }
};

class ConeGoal : public LinkGoalBase {  // :646-712
    Vector3 position, axis, direction;
    double position_weight = 0, angle = 0;

public:
    ConeGoal() : position(0, 0, 0), axis(0, 0, 1), direction(0, 0, 1) {}
    ConeGoal(const std::string& link_name, const Vector3& axis_, const Vector3& direction_, double angle_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), position(0, 0, 0), axis(axis_), direction(direction_), angle(angle_) {}
    ConeGoal(const std::string& link_name, const Vector3& position_, const Vector3& axis_, const Vector3& direction_, double angle_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), position(position_), axis(axis_), direction(direction_), position_weight(1), angle(angle_) {}
    ConeGoal(const std::string& link_name, const Vector3& position_, double position_weight_, const Vector3& axis_, const Vector3& direction_, double angle_,
             double weight = 1.0)
        : LinkGoalBase(link_name, weight), position(position_), axis(axis_), direction(direction_), position_weight(position_weight_), angle(angle_) {}
    const Vector3& getPosition() const { return position; }
    double getPositionWeight() const { return position_weight; }
    const Vector3& getAxis() const { return axis; }
    const Vector3& getDirection() const { return direction; }
    double getAngle() const { return angle; }
    void setPosition(const Vector3& p) { position = p; }
    void setPositionWeight(double w) { position_weight = w; }
    void setAxis(const Vector3& a) { axis = a.normalized(); }
    void setDirection(const Vector3& d) { direction = d.normalized(); }
    void setAngle(double a) { angle = a; }
    double evaluate(const GoalContext& context) const override {
        const Frame f = goalFrame(context);
        const Vector3 v = quatRotate(f.getOrientation(), axis);
        const double c = v.dot(direction) / std::sqrt(v.length2() * direction.length2());
        const double d = std::fmax(0.0, std::acos(std::fmin(1.0, std::fmax(-1.0, c))) - angle);
        return d * d + position_weight * position_weight * (position - f.getPosition()).length2();
    }
    int gpuOpcode() const override { return BIOIK_GOAL_CONE; }
    void gpuParams(std::vector<double>& o) const override {
        o.insert(o.end(), {position.x(), position.y(), position.z(), position_weight, axis.x(), axis.y(), axis.z(), direction.x(), direction.y(), direction.z(), angle});
    }
};

// TouchGoal (:330-377, goal_types.cpp:45-229): the collision shapes of the link touch the plane through `position` with `normal`.  No FCL: the shapes are the
// link's collision points x y z r and disks cx cy cz r ax ay az 0 of the robot model (RobotModel::addCollisionBox / Sphere / Points / Cylinder / Cone, the
// URDF reader, or LinkModel::getShapes() in the MoveIt plugin), and the cost is the squared support distance of their hull along the normal
// (include/bioik_hip.h: BIOIK_GOAL_TOUCH)
class TouchGoal : public LinkGoalBase {
    Vector3 position, normal;

public:
    TouchGoal() : position(0, 0, 0), normal(0, 0, 0) {}
    TouchGoal(const std::string& link_name, const Vector3& position_, const Vector3& normal_, double weight = 1.0)
        : LinkGoalBase(link_name, weight), position(position_), normal(normal_.normalized()) {}
    const Vector3& getPosition() const { return position; }
    const Vector3& getNormal() const { return normal; }
    // d = min(min_i (n_l . v_i - r_i), min_j (n_l . c_j - r_j |n_l x a_j|)) - normal . (position - p), n_l = the normal turned by the conjugate of the link's quaternion (tf2's inverse(), goal_types.cpp:170)
    static double distance(const Frame& fb, const Vector3& position, const Vector3& normal, const std::vector<double>& points,
                           const std::vector<double>& disks = std::vector<double>(), const std::vector<double>& capsules = std::vector<double>()) {
        const Quaternion q = fb.getOrientation();
        // v + 2 (w t + u x t), t = u x v with u = -q.xyz: the quaternion as it is, unit or not (frame.h:108-149)
        const Vector3 u(-q.x(), -q.y(), -q.z());
        const Vector3 t = u.cross(normal);
        const Vector3 nl = normal + (t * q.w() + u.cross(t)) * 2.0;
        double dmin = DBL_MAX;  // (a link without shapes: the reference's DBL_MAX, goal_types.cpp:154)
        for (size_t i = 0; i + 4 <= points.size(); i += 4) {
            if (points[i + 3] < 0) continue;  // (the marker of a shape that is no point set: the device refuses such a link)
            dmin = std::fmin(dmin, nl.x() * points[i] + nl.y() * points[i + 1] + nl.z() * points[i + 2] - points[i + 3]);
        }
        for (size_t i = 0; i + 8 <= disks.size(); i += 8) {  // a disk's support: the cross product, which keeps its digits where the normal is parallel to the axis
            const Vector3 rim = nl.cross(Vector3(disks[i + 4], disks[i + 5], disks[i + 6]));
            dmin = std::fmin(dmin, nl.x() * disks[i] + nl.y() * disks[i + 1] + nl.z() * disks[i + 2] - disks[i + 3] * std::sqrt(rim.dot(rim)));
        }
        for (size_t i = 0; i + 8 <= capsules.size(); i += 8)  // a capsule's support is the smaller of its two end spheres' (exact): the device reads it as those two points
            for (size_t e = 0; e < 8; e += 4) dmin = std::fmin(dmin, nl.x() * capsules[i + e] + nl.y() * capsules[i + e + 1] + nl.z() * capsules[i + e + 2] - capsules[i + 3]);
        return dmin - normal.dot(position - fb.getPosition());
    }
    double evaluate(const GoalContext& context) const override {
        const double d = distance(context.getLinkFrame(), position, normal, context.getLinkPoints(), context.getLinkDisks(), context.getLinkCapsules());
        return d * d;
    }
    int gpuOpcode() const override { return BIOIK_GOAL_TOUCH; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {position.x(), position.y(), position.z(), normal.x(), normal.y(), normal.z()}); }
};

// ClearanceGoal (no reference counterpart; include/bioik_hip.h: BIOIK_GOAL_CLEARANCE): the spheres of the link -- its collision points x y z r of the robot model -- keep
// at least `margin` away from a table of obstacle spheres cx cy cz R in the world frame (at most BIOIK_MAX_OBSTACLES rows):
//     w_i = p + rotate(q, v_i)     s_ij = (margin + r_i) + R_j     pen = s_ij > 0 ? max(0, s_ij - |w_i - c_j|) : 0     cost = sum_i sum_j pen^2
// The margin is a per-query number; the table is data of the goal, shared by every query of a call: the plugin core uploads it to the device when it differs from what
// the compiled problem holds (it is no part of the problem cache's key).  A link with disks or with a shape that is no set of spheres is refused by the device.
class ClearanceGoal : public LinkGoalBase {
    double margin_;
    std::vector<double> obstacles_;

public:
    ClearanceGoal() : margin_(0.0) {}
    ClearanceGoal(const std::string& link_name, double margin, const std::vector<double>& obstacles = std::vector<double>(), double weight = 1.0)
        : LinkGoalBase(link_name, weight), margin_(margin) {
        setObstacles(obstacles);
    }
    double getMargin() const { return margin_; }
    void setMargin(double m) { margin_ = m; }
    const std::vector<double>& getObstacles() const { return obstacles_; }
    void setObstacles(const std::vector<double>& rows) {  // cx cy cz R per obstacle: what bioik_problem_set_obstacles accepts
        if (rows.size() % 4 != 0) throw std::invalid_argument("ClearanceGoal: obstacle rows are cx cy cz R");
        if (rows.size() / 4 > (size_t)BIOIK_MAX_OBSTACLES) throw std::invalid_argument("ClearanceGoal: more than BIOIK_MAX_OBSTACLES obstacles");
        for (size_t i = 0; i < rows.size(); i++)
            if (!std::isfinite(rows[i]) || (i % 4 == 3 && rows[i] < 0)) throw std::invalid_argument("ClearanceGoal: an obstacle row must be finite with a radius >= 0");
        obstacles_ = rows;
    }
    void addObstacle(const Vector3& centre, double radius) {
        std::vector<double> rows = obstacles_;
        rows.insert(rows.end(), {centre.x(), centre.y(), centre.z(), radius});
        setObstacles(rows);
    }
    // CAPSULES (include/bioik_hip.h), restated on the host with plain multiplications and additions where the device fuses them: equal up to rounding
    static Vector3 carry(const Frame& fb, const Vector3& v) {  // p + rotate(q, v), q as it is
        const Quaternion q = fb.getOrientation();
        const Vector3 u(q.x(), q.y(), q.z());
        const Vector3 t = u.cross(v);
        return fb.getPosition() + v + (t * q.w() + u.cross(t)) * 2.0;
    }
    static double clamp01(double x) { return std::fmin(std::fmax(x, 0.0), 1.0); }
    static double segmentPointD2(const Vector3& a, const Vector3& b, const Vector3& c) {
        const Vector3 u = b - a, e = c - a;
        const double uu = u.dot(u), ru = uu > DBL_MIN ? 1.0 / uu : 0.0;
        const Vector3 x = c - (a + u * clamp01(e.dot(u) * ru));
        return x.dot(x);
    }
    static double segmentSegmentD2(const Vector3& a, const Vector3& b, const Vector3& c, const Vector3& d) {
        const Vector3 u = b - a, v = d - c, w = a - c;
        const double uu = u.dot(u), vv = v.dot(v), uv = u.dot(v), uw = u.dot(w), vw = v.dot(w);
        const double ru = uu > DBL_MIN ? 1.0 / uu : 0.0, rv = vv > DBL_MIN ? 1.0 / vv : 0.0;
        const double den = uu * vv - uv * uv;
        double s = den > 0.0 ? clamp01((uv * vw - vv * uw) / den) : 0.0;
        const double t = (uv * s + vw) * rv, tc = clamp01(t);
        if (tc != t || rv == 0.0) s = clamp01((uv * tc - uw) * ru);
        const Vector3 x = (a + u * s) - (c + v * tc);
        return x.dot(x);
    }
    static double tail(double sum, double s, double d2) {
        if (s > 0 && d2 < s * s) {
            const double pen = std::fmax(0.0, s - std::sqrt(d2));
            sum += pen * pen;
        }
        return sum;
    }
    // the pairs that involve a capsule: the link's points, then its capsules, each against the other side's points (`obstacles`) and then its capsules (taken as they are)
    static double capsuleCost(double sum, const Frame& fb, double margin, const std::vector<double>& points, const std::vector<double>& capsules, const std::vector<double>& obstacles,
                              const std::vector<double>& other_capsules) {
        for (size_t i = 0; i + 4 <= points.size() && !other_capsules.empty(); i += 4) {
            if (points[i + 3] < 0) continue;
            const Vector3 w = carry(fb, Vector3(points[i], points[i + 1], points[i + 2]));
            for (size_t j = 0; j + 8 <= other_capsules.size(); j += 8) {
                const double* o = &other_capsules[j];
                sum = tail(sum, (margin + points[i + 3]) + o[3], segmentPointD2(Vector3(o[0], o[1], o[2]), Vector3(o[4], o[5], o[6]), w));
            }
        }
        for (size_t i = 0; i + 8 <= capsules.size(); i += 8) {
            const double* k = &capsules[i];
            const Vector3 a = carry(fb, Vector3(k[0], k[1], k[2])), b = carry(fb, Vector3(k[4], k[5], k[6]));
            for (size_t j = 0; j + 4 <= obstacles.size(); j += 4)
                sum = tail(sum, (margin + k[3]) + obstacles[j + 3], segmentPointD2(a, b, Vector3(obstacles[j], obstacles[j + 1], obstacles[j + 2])));
            for (size_t j = 0; j + 8 <= other_capsules.size(); j += 8) {
                const double* o = &other_capsules[j];
                sum = tail(sum, (margin + k[3]) + o[3], segmentSegmentD2(a, b, Vector3(o[0], o[1], o[2]), Vector3(o[4], o[5], o[6])));
            }
        }
        return sum;
    }
    // with capsules: the point pairs as below, then the pairs that involve a capsule (opcode 19: `other_capsules` empty; the order of summation differs from the device's
    // where both links of a SelfClearanceGoal carry points AND capsules: equal up to rounding)
    static double cost(const Frame& fb, double margin, const std::vector<double>& points, const std::vector<double>& obstacles, const std::vector<double>& capsules,
                       const std::vector<double>& other_capsules = std::vector<double>()) {
        return capsuleCost(cost(fb, margin, points, obstacles), fb, margin, points, capsules, obstacles, other_capsules);
    }
    // the formula above with the quaternion as it is, unit or not (frame.h:108-149): i outer, j inner, one running sum
    static double cost(const Frame& fb, double margin, const std::vector<double>& points, const std::vector<double>& obstacles) {
        const Quaternion q = fb.getOrientation();
        const Vector3 u(q.x(), q.y(), q.z()), p = fb.getPosition();
        double sum = 0.0;
        for (size_t i = 0; i + 4 <= points.size(); i += 4) {
            if (points[i + 3] < 0) continue;  // (the marker of a shape that is no point set: the device refuses such a link)
            const Vector3 v(points[i], points[i + 1], points[i + 2]);
            const Vector3 t = u.cross(v);
            const Vector3 w = p + v + (t * q.w() + u.cross(t)) * 2.0;
            const double sm = margin + points[i + 3];
            for (size_t j = 0; j + 4 <= obstacles.size(); j += 4) {
                const double s = sm + obstacles[j + 3];
                const Vector3 e = Vector3(obstacles[j], obstacles[j + 1], obstacles[j + 2]) - w;
                const double d2 = e.dot(e);
                if (s > 0 && d2 < s * s) {
                    const double pen = std::fmax(0.0, s - std::sqrt(d2));
                    sum += pen * pen;
                }
            }
        }
        return sum;
    }
    double evaluate(const GoalContext& context) const override { return cost(context.getLinkFrame(), margin_, context.getLinkPoints(), obstacles_, context.getLinkCapsules()); }
    int gpuOpcode() const override { return BIOIK_GOAL_CLEARANCE; }
    void gpuParams(std::vector<double>& o) const override { o.push_back(margin_); }
    const std::vector<double>* gpuObstacles() const override { return &obstacles_; }
};

// SelfClearanceGoal (no reference counterpart; include/bioik_hip.h: BIOIK_GOAL_SELF_CLEARANCE): the spheres of the link keep at least `margin` away from the spheres
// of ANOTHER link of the same robot -- self-collision between two links.  The other link is the goal's base link (BASE LINKS): describe() adds both links, and the
// cost is ClearanceGoal's on R = concat(inverse(other), link) with the other link's collision points as the obstacle table.  Both tables are the robot model's.
class SelfClearanceGoal : public LinkGoalBase {
    double margin_;

public:
    SelfClearanceGoal() : margin_(0.0) {}
    SelfClearanceGoal(const std::string& link_name, const std::string& other_link, double margin = 0.0, double weight = 1.0) : LinkGoalBase(link_name, weight), margin_(margin) {
        setBaseLinkName(other_link);
    }
    double getMargin() const { return margin_; }
    void setMargin(double m) { margin_ = m; }
    void setOtherLinkName(const std::string& n) { setBaseLinkName(n); }
    const std::string& getOtherLinkName() const { return getBaseLinkName(); }
    // (reads both frames and both links' points: the hybrid path scores candidates with it)
    double evaluate(const GoalContext& context) const override {
        if (getBaseLinkName().empty()) return 0.0;  // (no other link: the device refuses such a goal)
        return ClearanceGoal::cost(goalFrame(context), margin_, context.getLinkPoints(0), context.getLinkPoints(1), context.getLinkCapsules(0), context.getLinkCapsules(1));
    }
    int gpuOpcode() const override { return BIOIK_GOAL_SELF_CLEARANCE; }
    void gpuParams(std::vector<double>& o) const override { o.push_back(margin_); }
};

class BalanceGoal : public Goal {  // goal_types.h:540-566, goal_types.cpp:231-272
    Vector3 target_, axis_;

public:
    BalanceGoal() : target_(0, 0, 0), axis_(0, 0, 1) {}
    BalanceGoal(const Vector3& target, double weight = 1.0) : target_(target), axis_(0, 0, 1) { weight_ = weight; }
    const Vector3& getTarget() const { return target_; }
    const Vector3& getAxis() const { return axis_; }
    void setTarget(const Vector3& target) { target_ = target; }
    void setAxis(const Vector3& axis) { axis_ = axis; }
    // (its cost reads every link with a mass: evaluated on the device only, where the problem compiler knows the model's inertials;
    // the host-side evaluate() of this build returns 0 for it)
    int gpuOpcode() const override { return BIOIK_GOAL_BALANCE; }
    void gpuParams(std::vector<double>& o) const override { o.insert(o.end(), {target_.x(), target_.y(), target_.z(), axis_.x(), axis_.y(), axis_.z()}); }
};

}  // namespace bio_ik
