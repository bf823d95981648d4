// MoveIt's multi-solution KinematicsBase::getPositionIK(ik_poses, ik_seed_state, solutions, result, options) of the plugin translation unit
// (bio_ik_amd/cpp/src/kinematics_plugin_hip.cpp), called through a kinematics::KinematicsBase* created by its pluginlib name: the count against the yaml key
// gpu_solutions, solution_percentage = returned successes / gpu_solutions, kinematic_error, every solution at the pose and apart from the others by more than
// gpu_solution_distance; then the batched free function searchPositionIKRanked and the refusal of callback goals.
#include <chrono>
#include <cstdio>
#include <fstream>
#include <random>
#include <sstream>

#include <moveit/kinematics_base/kinematics_base.h>
#include <moveit/rdf_loader/rdf_loader.h>
#include <pluginlib/class_list_macros.h>
#include <ros/ros.h>

#define BIOIK_WITH_KINEMATICS_BASE 1
#include <bio_ik/bio_ik.h>
#include <bio_ik/kinematics_plugin_hip.h>

#ifndef TEST_TIMEOUT
#define TEST_TIMEOUT 0.25
#endif
// budget of the solves that cannot succeed (an unreachable pose): a fifth of it on a GPU, two seconds of wall clock on the host simulator
#define TEST_FAR_TIMEOUT (TEST_TIMEOUT > 10.0 ? 2.0 : TEST_TIMEOUT * 0.2)

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static moveit::core::RobotModelPtr pr2Arm() {
    moveit::core::RobotModelPtr m(new moveit::core::RobotModel());
    m->addLink("base_footprint", "", "root_joint", "fixed", 0, 0, 0, 0, 0, 0, 0, 0, 1);
    m->addLink("base_link", "base_footprint", "base_footprint_joint", "fixed", 0, 0, 0.051, 0, 0, 0, 0, 0, 1);
    m->addLink("torso_lift_link", "base_link", "torso_lift_joint", "prismatic", -0.05, 0, 0.739675, 0, 0, 0, 0, 0, 1, 0.0, 0.33, 0.013);
    m->addLink("r_shoulder_pan_link", "torso_lift_link", "r_shoulder_pan_joint", "revolute", 0, -0.188, 0, 0, 0, 0, 0, 0, 1, -2.2854, 0.7146, 2.088);
    m->addLink("r_shoulder_lift_link", "r_shoulder_pan_link", "r_shoulder_lift_joint", "revolute", 0.1, 0, 0, 0, 0, 0, 0, 1, 0, -0.5236, 1.3963, 2.082);
    m->addLink("r_upper_arm_roll_link", "r_shoulder_lift_link", "r_upper_arm_roll_joint", "revolute", 0, 0, 0, 0, 0, 0, 1, 0, 0, -3.9, 0.8, 3.27);
    m->addLink("r_upper_arm_link", "r_upper_arm_roll_link", "r_upper_arm_joint", "fixed", 0, 0, 0, 0, 0, 0, 0, 0, 1);
    m->addLink("r_elbow_flex_link", "r_upper_arm_link", "r_elbow_flex_joint", "revolute", 0.4, 0, 0, 0, 0, 0, 0, 1, 0, -2.3213, 0.0, 3.3);
    m->addLink("r_forearm_roll_link", "r_elbow_flex_link", "r_forearm_roll_joint", "continuous", 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 3.6);
    m->addLink("r_forearm_link", "r_forearm_roll_link", "r_forearm_joint", "fixed", 0, 0, 0, 0, 0, 0, 0, 0, 1);
    m->addLink("r_wrist_flex_link", "r_forearm_link", "r_wrist_flex_joint", "revolute", 0.321, 0, 0, 0, 0, 0, 0, 1, 0, -2.18, 0.0, 3.078);
    m->addLink("r_wrist_roll_link", "r_wrist_flex_link", "r_wrist_roll_joint", "continuous", 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 3.6);
    m->addChainGroup("right_arm", "torso_lift_link", "r_wrist_roll_link");
    return m;
}

static geometry_msgs::Pose poseInBase(const moveit::core::RobotState& st, const std::string& base, const std::string& tip) {
    const Eigen::Isometry3d B = st.getGlobalLinkTransform(base), T = st.getGlobalLinkTransform(tip);
    Eigen::Isometry3d Bi;  // inverse of a rigid transform
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Bi.linear()(i, j) = B.linear()(j, i);
    const Eigen::Vector3d bt = Bi.linear() * B.translation();
    Bi.translation() = Eigen::Vector3d(-bt.x(), -bt.y(), -bt.z());
    const Eigen::Isometry3d R = Bi * T;
    const Eigen::Quaterniond q(R.rotation());
    geometry_msgs::Pose p;
    p.position.x = R.translation().x(), p.position.y = R.translation().y(), p.position.z = R.translation().z();
    p.orientation.x = q.x(), p.orientation.y = q.y(), p.orientation.z = q.z(), p.orientation.w = q.w();
    return p;
}


int main() {
    const int k = 4;
    const double distance = 0.1;
    ros::set_param("mode", "bio2_memetic");
    ros::set_param("random_seed", 3);
    ros::set_param("gpu_population", 16);
    ros::set_param("gpu_fk", "linear");
    ros::set_param("gpu_max_steps", 80);
    ros::set_param("gpu_islands", 6);
    ros::set_param("gpu_solutions", k);
    ros::set_param("gpu_solution_distance", distance);
    std::unique_ptr<kinematics::KinematicsBase> solver(static_cast<kinematics::KinematicsBase*>(pluginlib_standin_create("bio_ik_kinematics_plugin::BioIKKinematicsPlugin")));
    CHECK(solver != nullptr);
    moveit::core::RobotModelPtr rm = pr2Arm();
    CHECK(solver->initialize(*rm, "right_arm", "torso_lift_link", std::vector<std::string>{"r_wrist_roll_link"}, 0.0));
    std::mt19937 rng(5);
    auto uniform = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    moveit::core::RobotState target(rm), check(rm);
    std::vector<geometry_msgs::Pose> poses;
    std::vector<std::vector<double>> seeds;
    for (int q = 0; q < 2; q++) {
        target.setToDefaultValues();
        std::vector<double> seed;
        for (auto& jn : solver->getJointNames()) {
            const auto& b = rm->getVariableBounds(jn);
            const double v = uniform(b.min_position_, b.max_position_);
            target.setVariablePosition(jn, v);
            seed.push_back(std::min(std::max(v + uniform(-0.2, 0.2), b.min_position_), b.max_position_));
        }
        poses.push_back(poseInBase(target, "torso_lift_link", "r_wrist_roll_link"));
        seeds.push_back(seed);
    }
    auto tipError = [&](const std::vector<double>& solution, const geometry_msgs::Pose& want) {
        check.setToDefaultValues();
        for (size_t i = 0; i < solution.size(); i++) check.setVariablePosition(solver->getJointNames()[i], solution[i]);
        const geometry_msgs::Pose got = poseInBase(check, "torso_lift_link", "r_wrist_roll_link");
        const double dx = got.position.x - want.position.x, dy = got.position.y - want.position.y, dz = got.position.z - want.position.z;
        const double dot = std::fabs(got.orientation.x * want.orientation.x + got.orientation.y * want.orientation.y + got.orientation.z * want.orientation.z +
                                     got.orientation.w * want.orientation.w);
        return std::max(std::sqrt(dx * dx + dy * dy + dz * dz) / 1e-4, 2 * std::acos(std::min(1.0, dot)) / 1e-3);  // in units of the tolerance
    };
    auto apart = [&](const std::vector<std::vector<double>>& rows) {
        for (size_t a = 0; a < rows.size(); a++)
            for (size_t b = 0; b < a; b++) {
                double d = 0.0;
                for (size_t i = 0; i < rows[a].size(); i++) d = std::max(d, std::fabs(rows[a][i] - rows[b][i]));
                if (!(d > distance)) return false;
            }
        return true;
    };
    // the override, through the base class
    {
        std::vector<std::vector<double>> solutions;
        kinematics::KinematicsResult result;
        CHECK(solver->getPositionIK(std::vector<geometry_msgs::Pose>{poses[0]}, seeds[0], solutions, result, kinematics::KinematicsQueryOptions()));
        CHECK(result.kinematic_error == kinematics::KinematicError::OK);
        CHECK(solutions.size() >= 1 && solutions.size() <= (size_t)k);
        CHECK(std::fabs(result.solution_percentage - (double)solutions.size() / k) < 1e-12);  // (every returned row passed: no approximate ones were asked for)
        for (auto& s : solutions) CHECK(s.size() == 7 && tipError(s, poses[0]) < 1.0);
        CHECK(apart(solutions));
    }
    // the batched free function
    {
        std::vector<std::vector<std::vector<double>>> solutions;
        std::vector<moveit_msgs::MoveItErrorCodes> codes;
        CHECK(bio_ik_kinematics_plugin::searchPositionIKRanked(*solver, {{poses[0]}, {poses[1]}}, seeds, 3, distance, 0.0, solutions, codes));
        CHECK(solutions.size() == 2 && codes.size() == 2);
        for (size_t q = 0; q < 2; q++) {
            CHECK(codes[q].val == moveit_msgs::MoveItErrorCodes::SUCCESS && solutions[q].size() >= 1 && solutions[q].size() <= 3 && apart(solutions[q]));
            for (auto& s : solutions[q]) CHECK(tipError(s, poses[q]) < 1.0);
        }
    }
    // a callback goal: refused (no solutions through the interface, an exception from the free function)
    {
        bio_ik::BioIKKinematicsQueryOptions opts;
        opts.goals.emplace_back(new bio_ik::JointFunctionGoal(std::vector<std::string>{"r_elbow_flex_joint"}, [](std::vector<double>&) {}));
        std::vector<std::vector<double>> solutions;
        kinematics::KinematicsResult result;
        CHECK(!solver->getPositionIK(std::vector<geometry_msgs::Pose>{poses[0]}, seeds[0], solutions, result, opts));
        CHECK(result.kinematic_error == kinematics::KinematicError::NO_SOLUTION && solutions.empty() && result.solution_percentage == 0.0);
        bool threw = false;
        try {
            std::vector<std::vector<std::vector<double>>> s3;
            std::vector<moveit_msgs::MoveItErrorCodes> codes;
            bio_ik_kinematics_plugin::searchPositionIKRanked(*solver, {{poses[0]}}, {seeds[0]}, 3, distance, 0.0, s3, codes, opts);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
    }
    std::printf("ok\n");
    return 0;
}
