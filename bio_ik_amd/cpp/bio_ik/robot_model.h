// bio_ik/robot_model.h — flat robot description for the C-ABI (stand-in for what the reference reads from
// moveit::core::RobotModel / JointModelGroup: src/forward_kinematics.h:192-213, include/bio_ik/robot_info.h:70-106,
// src/problem.cpp:117-124,201-204).  With MoveIt available the same arrays are filled from a RobotModel.
#pragma once
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include <bioik_hip.h>

namespace bio_ik {

struct JointModelGroup {
    std::string name;
    std::vector<int32_t> active_joints;  // link indices, getActiveJointModels() order
    std::vector<int32_t> tips;
};

class RobotModel {
public:
    std::vector<std::string> link_names, joint_names, variable_names;
    std::vector<int32_t> link_parent, joint_type, joint_first_variable, joint_mimic;
    std::vector<double> link_origin, joint_axis, joint_mimic_factor, joint_mimic_offset, var_min, var_max, var_max_velocity;
    std::vector<double> link_mass, link_center;  // urdf <inertial> mass / origin xyz per link (BalanceGoal); empty = none
    std::vector<uint8_t> var_bounded;
    std::map<std::string, JointModelGroup> groups;
    // collision shapes as points (TouchGoal): per link rows x y z r in the link frame; r < 0 marks a shape that is no point set (a cylinder)
    std::map<int, std::vector<double>> link_points;
    struct MeshRef {  // a <mesh> collision a URDF names: its file is not loaded, the caller supplies the vertices (addCollisionPoints)
        std::string filename;
        double scale[3], origin[7];
        bool resolved = false;  // set once vertices were added for the link
    };
    std::map<int, std::vector<MeshRef>> link_meshes;
    // cylinders and cones: the convex hull of disks and points -- per link rows cx cy cz r ax ay az 0 in the link frame (the ends of cylinders, the bases of cones)
    std::map<int, std::vector<double>> link_disks;
    struct SolidRef {  // a <cylinder> collision a URDF names: left as a marker row until resolveCollisionSolids() turns it into its disks
        std::string kind;
        double radius, length, origin[7];
    };
    std::map<int, std::vector<SolidRef>> link_solids;
    // capsules: per link rows ax ay az r bx by bz 0 in the link frame -- a segment's two ends and a radius (ClearanceGoal, SelfClearanceGoal; TouchGoal reads each as two spheres)
    std::map<int, std::vector<double>> link_capsules;
    mutable std::vector<int32_t> point_first_, disk_first_, capsule_first_;  // flattened by desc()
    mutable std::vector<double> points_flat_, disks_flat_, capsules_flat_;

    // points (x y z triples) with radii (empty: all 0), moved by the shape's collision origin (px py pz qx qy qz qw; null or the identity: untouched)
    void addCollisionPoints(const std::string& link, const std::vector<double>& xyz, const std::vector<double>& radii = {}, const double* origin = nullptr) {
        std::vector<double>& t = link_points[linkIndex(link)];
        const bool ident = !origin || (origin[0] == 0 && origin[1] == 0 && origin[2] == 0 && origin[3] == 0 && origin[4] == 0 && origin[5] == 0 && origin[6] == 1);
        for (size_t i = 0; i + 3 <= xyz.size(); i += 3) {
            double v[3] = {xyz[i], xyz[i + 1], xyz[i + 2]};
            if (!ident) {
                double r[3];
                rotate(origin + 3, v, r);
                for (int c = 0; c < 3; c++) v[c] = r[c] + origin[c];
            }
            const double rad = radii.empty() ? 0.0 : radii[i / 3];
            if (!(rad >= 0)) throw std::runtime_error("collision radii must be >= 0");
            t.insert(t.end(), {v[0], v[1], v[2], rad});
        }
        auto mr = link_meshes.find(linkIndex(link));
        if (mr != link_meshes.end())
            for (MeshRef& r : mr->second) r.resolved = true;
    }
    void addCollisionBox(const std::string& link, const double (&size)[3], const double* origin = nullptr) {  // its 8 corners (exact)
        std::vector<double> c;
        for (int sx = -1; sx <= 1; sx += 2)
            for (int sy = -1; sy <= 1; sy += 2)
                for (int sz = -1; sz <= 1; sz += 2) c.insert(c.end(), {sx * 0.5 * size[0], sy * 0.5 * size[1], sz * 0.5 * size[2]});
        const bool keep = meshesResolved(link);
        addCollisionPoints(link, c, {}, origin);
        if (!keep) unresolveMeshes(link);
    }
    void addCollisionSphere(const std::string& link, double radius, const double* origin = nullptr) {  // one point with a radius (exact)
        const bool keep = meshesResolved(link);
        addCollisionPoints(link, {0.0, 0.0, 0.0}, {radius}, origin);
        if (!keep) unresolveMeshes(link);
    }
    // raw disks: rows cx cy cz r ax ay az 0 (radius >= 0, axis of unit length within 1e-9), centres moved and axes turned by the shape's collision origin
    void addCollisionDisks(const std::string& link, const std::vector<double>& rows, const double* origin = nullptr) {
        std::vector<double>& t = link_disks[linkIndex(link)];
        const bool ident = !origin || (origin[0] == 0 && origin[1] == 0 && origin[2] == 0 && origin[3] == 0 && origin[4] == 0 && origin[5] == 0 && origin[6] == 1);
        for (size_t i = 0; i + 8 <= rows.size(); i += 8) {
            double c[3] = {rows[i], rows[i + 1], rows[i + 2]}, a[3] = {rows[i + 4], rows[i + 5], rows[i + 6]};
            const double len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
            if (!(rows[i + 3] >= 0) || !(std::fabs(len - 1.0) <= 1e-9) || rows[i + 7] != 0) throw std::runtime_error("collision disks: radius >= 0, a unit axis, an eighth number 0");
            if (!ident) {
                double r[3];
                rotate(origin + 3, c, r);
                for (int k = 0; k < 3; k++) c[k] = r[k] + origin[k];
                rotate(origin + 3, a, r);
                for (int k = 0; k < 3; k++) a[k] = r[k];
            }
            t.insert(t.end(), {c[0], c[1], c[2], rows[i + 3], a[0], a[1], a[2], 0.0});
        }
    }
    // raw capsules: rows ax ay az r bx by bz 0 (radius >= 0, the two ends different: a sphere is a point row), both ends moved by the shape's collision origin
    void addCollisionCapsules(const std::string& link, const std::vector<double>& rows, const double* origin = nullptr) {
        std::vector<double>& t = link_capsules[linkIndex(link)];
        const bool ident = !origin || (origin[0] == 0 && origin[1] == 0 && origin[2] == 0 && origin[3] == 0 && origin[4] == 0 && origin[5] == 0 && origin[6] == 1);
        for (size_t i = 0; i + 8 <= rows.size(); i += 8) {
            double a[3] = {rows[i], rows[i + 1], rows[i + 2]}, b[3] = {rows[i + 4], rows[i + 5], rows[i + 6]};
            for (int c = 0; c < 8; c++)
                if (!std::isfinite(rows[i + c])) throw std::runtime_error("collision capsules must be finite");
            if (!(rows[i + 3] >= 0) || rows[i + 7] != 0) throw std::runtime_error("collision capsules: radius >= 0, an eighth number 0");
            if (a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) throw std::runtime_error("collision capsules: the two ends coincide (a sphere is a point row: addCollisionSphere)");
            if (!ident) {
                double r[3];
                rotate(origin + 3, a, r);
                for (int k = 0; k < 3; k++) a[k] = r[k] + origin[k];
                rotate(origin + 3, b, r);
                for (int k = 0; k < 3; k++) b[k] = r[k] + origin[k];
            }
            t.insert(t.end(), {a[0], a[1], a[2], rows[i + 3], b[0], b[1], b[2], 0.0});
        }
    }
    // a capsule centred on its origin with its axis along z; `length` is the SEGMENT's length (the capsule is length + 2 radius long overall)
    void addCollisionCapsule(const std::string& link, double radius, double length, const double* origin = nullptr) {
        addCollisionCapsules(link, {0.0, 0.0, -0.5 * length, radius, 0.0, 0.0, 0.5 * length, 0.0}, origin);
    }
    const std::vector<double>* collisionCapsules(const std::string& link) const {
        auto it = link_capsules.find(linkIndex(link));
        return it == link_capsules.end() ? nullptr : &it->second;
    }
    // URDF <cylinder> / shapes::Cylinder: centred on its origin, axis z -- its two end disks (exact: a cylinder is their convex hull)
    void addCollisionCylinder(const std::string& link, double radius, double length, const double* origin = nullptr) {
        addCollisionDisks(link, {0.0, 0.0, -0.5 * length, radius, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.5 * length, radius, 0.0, 0.0, 1.0, 0.0}, origin);
    }
    // shapes::Cone of MoveIt: the origin halfway up, the tip on +z -- its base disk and its apex as a point with r = 0 (exact)
    void addCollisionCone(const std::string& link, double radius, double length, const double* origin = nullptr) {
        addCollisionDisks(link, {0.0, 0.0, -0.5 * length, radius, 0.0, 0.0, 1.0, 0.0}, origin);
        const bool keep = meshesResolved(link);
        addCollisionPoints(link, {0.0, 0.0, 0.5 * length}, {}, origin);
        if (!keep) unresolveMeshes(link);
    }
    void addCollisionSolidRef(const std::string& link, const std::string& kind, double radius, double length, const double (&origin)[7]) {
        SolidRef r;
        r.kind = kind, r.radius = radius, r.length = length;
        for (int c = 0; c < 7; c++) r.origin[c] = origin[c];
        link_solids[linkIndex(link)].push_back(r);
    }
    // every solid the URDF reader recorded (of `link`, or of all links) becomes its disks, and exactly the marker row the reader left for it goes.
    // cylinders = "capsule": a cylinder becomes its BOUNDING CAPSULE instead (the same radius, the segment its whole axis), which ClearanceGoal and SelfClearanceGoal can
    // measure -- an approximation asked for by name, never silent: it contains the cylinder and overshoots it by the radius at each end
    void resolveCollisionSolids(const std::string& link = "", const std::string& cylinders = "disks") {
        if (cylinders != "disks" && cylinders != "capsule") throw std::runtime_error("resolveCollisionSolids: cylinders is \"disks\" or \"capsule\"");
        for (auto& ls : link_solids) {
            if (!link.empty() && ls.first != linkIndex(link)) continue;
            const std::string& name = link_names[ls.first];
            for (const SolidRef& r : ls.second) {
                if (r.kind == "cylinder" && cylinders == "capsule") addCollisionCapsule(name, r.radius, r.length, r.origin);
                else if (r.kind == "cylinder") addCollisionCylinder(name, r.radius, r.length, r.origin);
                else addCollisionCone(name, r.radius, r.length, r.origin);
                std::vector<double>& t = link_points[ls.first];
                for (size_t i = 0; i + 4 <= t.size(); i += 4)
                    if (t[i + 3] < 0) {
                        t.erase(t.begin() + i, t.begin() + i + 4);
                        break;
                    }
            }
            ls.second.clear();
        }
    }
    const std::vector<double>* collisionDisks(const std::string& link) const {
        auto it = link_disks.find(linkIndex(link));
        return it == link_disks.end() ? nullptr : &it->second;
    }
    void addCollisionUnsupported(const std::string& link) {  // a shape nobody converted (a cylinder or a cone left as it was): a TouchGoal on this link is refused, never approximated
        link_points[linkIndex(link)].insert(link_points[linkIndex(link)].end(), {0.0, 0.0, 0.0, -1.0});
    }
    void addCollisionMeshRef(const std::string& link, const std::string& filename, const double (&scale)[3], const double (&origin)[7]) {
        MeshRef r;
        r.filename = filename;
        for (int c = 0; c < 3; c++) r.scale[c] = scale[c];
        for (int c = 0; c < 7; c++) r.origin[c] = origin[c];
        link_meshes[linkIndex(link)].push_back(r);
    }
    bool meshesResolved(const std::string& link) const {
        auto mr = link_meshes.find(linkIndex(link));
        if (mr == link_meshes.end()) return true;
        for (const MeshRef& r : mr->second)
            if (!r.resolved) return false;
        return true;
    }
    void unresolveMeshes(const std::string& link) {
        for (MeshRef& r : link_meshes[linkIndex(link)]) r.resolved = false;
    }
    const std::vector<double>* collisionPoints(const std::string& link) const {
        auto it = link_points.find(linkIndex(link));
        return it == link_points.end() ? nullptr : &it->second;
    }

    static void quatFromRpy(double r, double p, double y, double* q) {
        double cr = std::cos(r / 2), sr = std::sin(r / 2), cp = std::cos(p / 2), sp = std::sin(p / 2), cy = std::cos(y / 2), sy = std::sin(y / 2);
        q[0] = sr * cp * cy - cr * sp * sy, q[1] = cr * sp * cy + sr * cp * sy, q[2] = cr * cp * sy - sr * sp * cy, q[3] = cr * cp * cy + sr * sp * sy;
    }
    int linkIndex(const std::string& n) const {
        for (size_t i = 0; i < link_names.size(); i++)
            if (link_names[i] == n) return (int)i;
        throw std::runtime_error("link not found: " + n);  // reference problem.cpp:141
    }
    int jointIndex(const std::string& n) const {
        for (size_t i = 0; i < joint_names.size(); i++)
            if (joint_names[i] == n) return (int)i;
        throw std::runtime_error("joint not found: " + n);
    }
    int variableIndex(const std::string& n) const {
        for (size_t i = 0; i < variable_names.size(); i++)
            if (variable_names[i] == n) return (int)i;
        throw std::runtime_error("joint variable not found: " + n);  // reference problem.cpp:125
    }
    // type: "fixed" | "revolute" | "continuous" | "prismatic" (URDF semantics) | "floating" | "planar" (MoveIt's multi-variable joints:
    // variables <joint>/trans_x .. rot_w and <joint>/x, y, theta; the device takes one such joint, at the root of the model)
    int addLink(const std::string& link, const std::string& parent, const std::string& joint, const std::string& type, const double (&xyz)[3],
                const double (&rpy)[3], const double (&axis)[3], double lower = 0, double upper = 0, double velocity = 0) {
        int idx = (int)link_names.size();
        link_names.push_back(link);
        joint_names.push_back(joint.empty() ? link + "_joint" : joint);
        link_parent.push_back(parent.empty() ? -1 : linkIndex(parent));
        double q[4];
        quatFromRpy(rpy[0], rpy[1], rpy[2], q);
        for (double v : {xyz[0], xyz[1], xyz[2], q[0], q[1], q[2], q[3]}) link_origin.push_back(v);
        int t = type == "fixed" ? BIOIK_JOINT_FIXED : (type == "prismatic" ? BIOIK_JOINT_PRISMATIC : (type == "floating" ? BIOIK_JOINT_FLOATING : (type == "planar" ? BIOIK_JOINT_PLANAR : BIOIK_JOINT_REVOLUTE)));
        if (type != "fixed" && type != "prismatic" && type != "revolute" && type != "continuous" && type != "floating" && type != "planar")
            throw std::runtime_error("unsupported joint type " + type);
        joint_type.push_back(t);
        double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
        const bool has_axis = t == BIOIK_JOINT_REVOLUTE || t == BIOIK_JOINT_PRISMATIC;
        for (int c = 0; c < 3; c++) joint_axis.push_back(!has_axis || n == 0 ? axis[c] : axis[c] / n);
        joint_mimic.push_back(-1);
        joint_mimic_factor.push_back(1.0);
        joint_mimic_offset.push_back(0.0);
        auto variable = [&](const std::string& name, double lo, double hi, bool bounded) {
            variable_names.push_back(name), var_min.push_back(lo), var_max.push_back(hi), var_bounded.push_back(bounded ? 1 : 0), var_max_velocity.push_back(velocity);
        };
        if (t == BIOIK_JOINT_FIXED) {
            joint_first_variable.push_back(-1);
        } else if (t == BIOIK_JOINT_FLOATING) {  // MoveIt FloatingJointModel: position unbounded, quaternion components in [-1, 1]
            joint_first_variable.push_back((int)variable_names.size());
            for (const char* c : {"trans_x", "trans_y", "trans_z"}) variable(joint_names.back() + "/" + c, -1e300, 1e300, false);
            for (const char* c : {"rot_x", "rot_y", "rot_z", "rot_w"}) variable(joint_names.back() + "/" + c, -1.0, 1.0, true);
        } else if (t == BIOIK_JOINT_PLANAR) {  // PlanarJointModel: x, y unbounded, theta in [-pi, pi] and not position-bounded
            joint_first_variable.push_back((int)variable_names.size());
            variable(joint_names.back() + "/x", -1e300, 1e300, false), variable(joint_names.back() + "/y", -1e300, 1e300, false);
            variable(joint_names.back() + "/theta", -M_PI, M_PI, false);
        } else {
            joint_first_variable.push_back((int)variable_names.size());
            variable_names.push_back(joint_names.back());
            bool cont = type == "continuous";  // MoveIt: bounds [-pi, pi], position_bounded_ = false
            var_min.push_back(cont ? -M_PI : lower);
            var_max.push_back(cont ? M_PI : upper);
            var_bounded.push_back(cont ? 0 : 1);
            var_max_velocity.push_back(velocity);
        }
        return idx;
    }
    void setInertial(const std::string& link, double mass, double cx, double cy, double cz) {  // urdf <inertial>
        link_mass.resize(link_names.size(), 0.0), link_center.resize(3 * link_names.size(), 0.0);
        const int i = linkIndex(link);
        link_mass[i] = mass, link_center[3 * i] = cx, link_center[3 * i + 1] = cy, link_center[3 * i + 2] = cz;
    }
    void addChainGroup(const std::string& name, const std::string& base, const std::string& tip) {
        JointModelGroup g;
        g.name = name;
        std::vector<int32_t> links;
        for (int l = linkIndex(tip), b = linkIndex(base); l != b; l = link_parent[l]) {
            if (l < 0) throw std::runtime_error(base + " is not an ancestor of " + tip);
            links.insert(links.begin(), l);
        }
        for (int l : links)  // JointModelGroup::getActiveJointModels: neither fixed nor mimic joints
            if (joint_type[l] != BIOIK_JOINT_FIXED && joint_mimic[l] < 0) g.active_joints.push_back(l);
        g.tips.push_back(linkIndex(tip));
        groups[name] = g;
    }
    void addJointGroup(const std::string& name, const std::vector<std::string>& joints, const std::vector<std::string>& tips) {
        JointModelGroup g;
        g.name = name;
        for (auto& j : joints) g.active_joints.push_back(jointIndex(j));
        for (auto& t : tips) g.tips.push_back(linkIndex(t));
        groups[name] = g;
    }
    std::vector<double> defaultPositions() const {  // RobotModel::getVariableDefaultPositions
        std::vector<double> out(variable_names.size(), 0.0);
        for (size_t v = 0; v < out.size(); v++)
            if (!(var_min[v] <= 0.0 && 0.0 <= var_max[v])) out[v] = 0.5 * (var_min[v] + var_max[v]);
        for (size_t l = 0; l < joint_type.size(); l++)
            if (joint_type[l] == BIOIK_JOINT_FLOATING) out[joint_first_variable[l] + 6] = 1.0;  // identity quaternion
        return out;
    }
    // A joint that mimics a joint that itself mimics another follows the joint at the end of the chain with the composed factor and offset, as MoveIt's
    // RobotModel::buildMimic leaves every model: x = f1 (f2 y + o2) + o1 -> factor f1 f2, offset o1 + f1 o2 (the loaders call it once the joints exist)
    void resolveMimicChains() {
        for (size_t pass = 0; pass <= joint_mimic.size() + 1; pass++) {
            bool changed = false;
            for (size_t i = 0; i < joint_mimic.size(); i++) {
                const int32_t m = joint_mimic[i];
                if (m >= 0 && joint_mimic[m] >= 0) {
                    joint_mimic_offset[i] = joint_mimic_offset[i] + joint_mimic_factor[i] * joint_mimic_offset[m];
                    joint_mimic_factor[i] = joint_mimic_factor[i] * joint_mimic_factor[m];
                    joint_mimic[i] = joint_mimic[m];
                    changed = true;
                }
            }
            if (!changed) return;
        }
        throw std::runtime_error("mimic joints that follow each other in a circle");
    }
    bioik_model_desc desc() const {
        bioik_model_desc d{};
        d.struct_size = sizeof(d);
        d.n_links = (uint32_t)link_names.size();
        d.n_variables = (uint32_t)variable_names.size();
        d.link_parent = link_parent.data(), d.link_origin = link_origin.data(), d.joint_type = joint_type.data(), d.joint_axis = joint_axis.data();
        d.joint_first_variable = joint_first_variable.data(), d.joint_mimic = joint_mimic.data();
        d.joint_mimic_factor = joint_mimic_factor.data(), d.joint_mimic_offset = joint_mimic_offset.data();
        d.var_min = var_min.data(), d.var_max = var_max.data(), d.var_bounded = var_bounded.data(), d.var_max_velocity = var_max_velocity.data();
        if (link_mass.size() == link_names.size() && link_center.size() == 3 * link_names.size()) d.link_mass = link_mass.data(), d.link_center = link_center.data();
        point_first_.assign(1, 0), points_flat_.clear();
        for (size_t l = 0; l < link_names.size(); l++) {
            auto it = link_points.find((int)l);
            if (it != link_points.end()) points_flat_.insert(points_flat_.end(), it->second.begin(), it->second.end());
            // a <mesh> whose vertices nobody supplied: the link is marked like a shape without a point form, so a TouchGoal on it is refused and not scored on the rest
            auto mr = link_meshes.find((int)l);
            if (mr != link_meshes.end())
                for (const MeshRef& r : mr->second)
                    if (!r.resolved) {
                        points_flat_.insert(points_flat_.end(), {0.0, 0.0, 0.0, -1.0});
                        break;
                    }
            point_first_.push_back((int32_t)(points_flat_.size() / 4));
        }
        if (!points_flat_.empty()) d.link_point_first = point_first_.data(), d.link_points = points_flat_.data();
        disk_first_.assign(1, 0), disks_flat_.clear();
        for (size_t l = 0; l < link_names.size(); l++) {
            auto it = link_disks.find((int)l);
            if (it != link_disks.end()) disks_flat_.insert(disks_flat_.end(), it->second.begin(), it->second.end());
            disk_first_.push_back((int32_t)(disks_flat_.size() / 8));
        }
        if (!disks_flat_.empty()) d.link_disk_first = disk_first_.data(), d.link_disks = disks_flat_.data();
        capsule_first_.assign(1, 0), capsules_flat_.clear();
        for (size_t l = 0; l < link_names.size(); l++) {
            auto it = link_capsules.find((int)l);
            if (it != link_capsules.end()) capsules_flat_.insert(capsules_flat_.end(), it->second.begin(), it->second.end());
            capsule_first_.push_back((int32_t)(capsules_flat_.size() / 8));
        }
        if (!capsules_flat_.empty()) d.link_capsule_first = capsule_first_.data(), d.link_capsules = capsules_flat_.data();
        return d;
    }
    // frame algebra for the plugin boundary (goal poses into the model frame, kinematics_plugin.cpp:487-502)
    static void rotate(const double* q, const double* v, double* r) {
        double tx = 2 * (q[1] * v[2] - q[2] * v[1]), ty = 2 * (q[2] * v[0] - q[0] * v[2]), tz = 2 * (q[0] * v[1] - q[1] * v[0]);
        r[0] = v[0] + q[3] * tx + q[1] * tz - q[2] * ty;
        r[1] = v[1] + q[3] * ty + q[2] * tx - q[0] * tz;
        r[2] = v[2] + q[3] * tz + q[0] * ty - q[1] * tx;
    }
    static void concat(const double* a, const double* b, double* r) {
        double p[3];
        rotate(a + 3, b, p);
        double o[7] = {a[0] + p[0], a[1] + p[1], a[2] + p[2],
                       a[6] * b[3] + a[3] * b[6] + a[4] * b[5] - a[5] * b[4], a[6] * b[4] - a[3] * b[5] + a[4] * b[6] + a[5] * b[3],
                       a[6] * b[5] + a[3] * b[4] - a[4] * b[3] + a[5] * b[6], a[6] * b[6] - a[3] * b[3] - a[4] * b[4] - a[5] * b[5]};
        for (int i = 0; i < 7; i++) r[i] = o[i];
    }
    void linkTransform(int link, const std::vector<double>& positions, double* f) const {
        std::vector<int> chain;
        for (int l = link; l >= 0; l = link_parent[l]) chain.insert(chain.begin(), l);
        double cur[7] = {0, 0, 0, 0, 0, 0, 1};
        for (int l : chain) {
            concat(cur, &link_origin[7 * l], cur);
            if (joint_type[l] == BIOIK_JOINT_REVOLUTE) {
                double h = 0.5 * positions[joint_first_variable[l]], s = std::sin(h);
                double j[7] = {0, 0, 0, joint_axis[3 * l] * s, joint_axis[3 * l + 1] * s, joint_axis[3 * l + 2] * s, std::cos(h)};
                concat(cur, j, cur);
            } else if (joint_type[l] == BIOIK_JOINT_PRISMATIC) {
                double v = positions[joint_first_variable[l]];
                double j[7] = {joint_axis[3 * l] * v, joint_axis[3 * l + 1] * v, joint_axis[3 * l + 2] * v, 0, 0, 0, 1};
                concat(cur, j, cur);
            } else if (joint_type[l] == BIOIK_JOINT_FLOATING) {
                const double* v = &positions[joint_first_variable[l]];
                const double n = std::sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
                double j[7] = {v[0], v[1], v[2], v[3] / n, v[4] / n, v[5] / n, v[6] / n};
                concat(cur, j, cur);
            } else if (joint_type[l] == BIOIK_JOINT_PLANAR) {
                const double* v = &positions[joint_first_variable[l]];
                double j[7] = {v[0], v[1], 0, 0, 0, std::sin(0.5 * v[2]), std::cos(0.5 * v[2])};
                concat(cur, j, cur);
            }
        }
        for (int i = 0; i < 7; i++) f[i] = cur[i];
    }
};

}  // namespace bio_ik
