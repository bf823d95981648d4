// C++ driver of capsules as link collision shapes (bio_ik/robot_model.h: addCollisionCapsule; include/bioik_hip.h: CAPSULES), tests/test_cpp_capsules.py: the
// reference-style construction compiles, the host evaluate() of ClearanceGoal, SelfClearanceGoal and TouchGoal with capsules is compared against the device's cost and
// the difference printed, and one query is solved through the plugin core on a model built with addCollisionCapsule: the wrist's capsule keeps clear of the upper arm's.
#include <cmath>
#include <cstdio>
#include <random>

#include <bio_ik/bio_ik.h>
#include <bio_ik/goal_eval.h>
#include <bio_ik/kinematics_plugin.h>

#ifndef TEST_TIMEOUT
#define TEST_TIMEOUT 5.0
#endif
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bio_ik::RobotModel rightArm() {
    bio_ik::RobotModel m;
    const double z[3] = {0, 0, 0}, ax[3] = {1, 0, 0}, ay[3] = {0, 1, 0}, az[3] = {0, 0, 1};
    m.addLink("base_footprint", "", "", "fixed", z, z, az);
    m.addLink("base_link", "base_footprint", "base_footprint_joint", "fixed", {0, 0, 0.051}, z, az);
    m.addLink("torso_lift_link", "base_link", "torso_lift_joint", "prismatic", {-0.05, 0, 0.739675}, z, az, 0.0, 0.33, 0.013);
    m.addLink("r_shoulder_pan_link", "torso_lift_link", "r_shoulder_pan_joint", "revolute", {0, -0.188, 0}, z, az, -2.2854, 0.7146, 2.088);
    m.addLink("r_shoulder_lift_link", "r_shoulder_pan_link", "r_shoulder_lift_joint", "revolute", {0.1, 0, 0}, z, ay, -0.5236, 1.3963, 2.082);
    m.addLink("r_upper_arm_roll_link", "r_shoulder_lift_link", "r_upper_arm_roll_joint", "revolute", z, z, ax, -3.9, 0.8, 3.27);
    m.addLink("r_elbow_flex_link", "r_upper_arm_roll_link", "r_elbow_flex_joint", "revolute", {0.4, 0, 0}, z, ay, -2.3213, 0.0, 3.3);
    m.addLink("r_forearm_roll_link", "r_elbow_flex_link", "r_forearm_roll_joint", "continuous", z, z, ax, 0, 0, 3.6);
    m.addLink("r_wrist_flex_link", "r_forearm_roll_link", "r_wrist_flex_joint", "revolute", {0.321, 0, 0}, z, ay, -2.18, 0.0, 3.078);
    m.addLink("r_wrist_roll_link", "r_wrist_flex_link", "r_wrist_roll_joint", "continuous", z, z, ax, 0, 0, 3.6);
    m.addChainGroup("right_arm", "torso_lift_link", "r_wrist_roll_link");
    const double along_x[7] = {0.15, 0, 0, 0, std::sqrt(0.5), 0, std::sqrt(0.5)};  // a quarter turn about y: the capsule's z axis onto the link's x, centred at x = 0.15
    m.addCollisionCapsule("r_upper_arm_roll_link", 0.2, 0.1, along_x);  // (generous: a bent elbow brings the hand inside it)
    m.addCollisionCapsules("r_wrist_roll_link", {0.0, 0, 0, 0.04, 0.08, 0, 0, 0});
    m.addCollisionPoints("r_wrist_roll_link", {0.04, 0.0, 0.03}, {0.02});
    return m;
}

struct Device {
    bioik_model* model = nullptr;
    bioik_problem* problem = nullptr;
    std::vector<int32_t> active;
    ~Device() {
        if (problem) bioik_problem_destroy(problem);
        if (model) bioik_model_destroy(model);
    }
};

// host evaluate() (bio_ik/goal_eval.h, what the hybrid path scores with) against bioik_eval_fitness on n random configurations: the worst difference, or -1
static double against_device(const bio_ik::RobotModel& rm, const bio_ik::Goal& goal, bioik_goal_desc gd, int base, const std::vector<double>& par, const std::vector<double>& obstacles,
                             int& hits, int n = 100) {
    using namespace bio_ik;
    Device dev;
    bioik_model_desc md = rm.desc();
    if (bioik_model_create(&md, 0, &dev.model) != BIOIK_OK) return -1;
    std::vector<int32_t> bases{base};
    const JointModelGroup& jmg = rm.groups.at("right_arm");
    bioik_problem_desc pd{};
    pd.struct_size = sizeof(pd);
    pd.n_group_joints = (uint32_t)jmg.active_joints.size(), pd.group_joints = jmg.active_joints.data();
    pd.n_goals = 1, pd.goals = &gd, pd.goal_base_link = base >= 0 ? bases.data() : nullptr;
    if (bioik_problem_create(dev.model, &pd, &dev.problem) != BIOIK_OK) return -1;
    if (!obstacles.empty() && bioik_problem_set_obstacles(dev.problem, 0, obstacles.size() / 4, obstacles.data()) != BIOIK_OK) return -1;
    const int D = bioik_problem_active_variable_count(dev.problem);
    dev.active.resize(D);
    bioik_problem_active_variables(dev.problem, dev.active.data());
    HostGoalProblem::Model hm;
    for (size_t v = 0; v < rm.variable_names.size(); v++) hm.info.addVariable(rm.var_min[v], rm.var_max[v], rm.var_bounded[v] != 0, rm.var_max_velocity[v], true, false);
    hm.variable_index = [&](const std::string& s) { return rm.variableIndex(s); };
    hm.link_frame = [&](const std::string& s, const std::vector<double>& p) {
        double f[7];
        rm.linkTransform(rm.linkIndex(s), p, f);
        return Frame(Vector3(f[0], f[1], f[2]), Quaternion(f[3], f[4], f[5], f[6]));
    };
    hm.link_points = [&](const std::string& s) { return rm.collisionPoints(s); };
    hm.link_capsules = [&](const std::string& s) { return rm.collisionCapsules(s); };
    std::mt19937 rng(5);
    auto limit = [&](int v, bool hi) { return rm.var_bounded[v] ? (hi ? rm.var_max[v] : rm.var_min[v]) : (hi ? 3.0 : -3.0); };
    std::vector<double> seed = rm.defaultPositions();
    HostGoalProblem host(hm, {&goal}, std::vector<int>(dev.active.begin(), dev.active.end()), seed);
    double worst = 0;
    hits = 0;
    for (int k = 0; k < n; k++) {
        std::vector<double> x = seed, genes(D);
        for (int i = 0; i < D; i++) x[dev.active[i]] = genes[i] = std::uniform_real_distribution<double>(limit(dev.active[i], false), limit(dev.active[i], true))(rng);
        double d = 0, sec = 0;
        if (bioik_eval_fitness(dev.problem, BIOIK_FK_EXACT, 1, seed.data(), par.data(), nullptr, genes.data(), &d, &sec) != BIOIK_OK) return -1;
        const double fit = host.computeGoalFitness(x);
        if (!std::isfinite(d)) return -1;
        worst = std::fmax(worst, std::fabs(fit - d) / (1 + std::fabs(d)));
        hits += fit > 0;
    }
    return worst;
}

int main() {
    using namespace bio_ik;
    RobotModel rm = rightArm();
    const std::string UA = "r_upper_arm_roll_link", RW = "r_wrist_roll_link";
    {  // the model's capsules as the device will read them; the refusals of the setters; desc()
        const std::vector<double>* c = rm.collisionCapsules(UA);
        CHECK(c && c->size() == 8 && std::fabs((*c)[0] - 0.1) < 1e-15 && std::fabs((*c)[4] - 0.2) < 1e-15 && (*c)[3] == 0.2 && (*c)[7] == 0.0 && std::fabs((*c)[2]) < 1e-15);
        CHECK(rm.collisionCapsules(RW)->size() == 8 && rm.collisionCapsules("base_link") == nullptr);
        bool threw = false;
        try {
            rm.addCollisionCapsules(RW, {1, 2, 3, 0.1, 1, 2, 3, 0});
        } catch (const std::exception&) {
            threw = true;
        }
        CHECK(threw && rm.collisionCapsules(RW)->size() == 8);
        bioik_model_desc md = rm.desc();
        CHECK(md.struct_size == sizeof(bioik_model_desc) && md.link_capsule_first && md.link_capsules && md.link_capsule_first[rm.link_names.size()] == 2);
        RobotModel cyl = rightArm();
        const double ident[7] = {0, 0, 0, 0, 0, 0, 1};
        cyl.addCollisionSolidRef("r_forearm_roll_link", "cylinder", 0.05, 0.3, ident);
        cyl.addCollisionUnsupported("r_forearm_roll_link");
        cyl.resolveCollisionSolids("r_forearm_roll_link", "capsule");  // the bounding capsule, asked for by name
        const std::vector<double>* b = cyl.collisionCapsules("r_forearm_roll_link");
        CHECK(b && b->size() == 8 && (*b)[2] == -0.15 && (*b)[6] == 0.15 && (*b)[3] == 0.05 && cyl.collisionDisks("r_forearm_roll_link") == nullptr);
        CHECK(cyl.collisionPoints("r_forearm_roll_link")->empty());
    }
    {  // the reference's usage (goals pushed into BioIKKinematicsQueryOptions) is what it was: capsules are model data, the goals carry no new field
        BioIKKinematicsQueryOptions options;
        options.goals.emplace_back(new SelfClearanceGoal(RW, UA, 0.02, 0.5));
        options.goals.emplace_back(new ClearanceGoal(RW, 0.01, {0.5, -0.2, 0.8, 0.1}));
        options.goals.emplace_back(new TouchGoal(RW, Vector3(0.5, -0.2, 0.7), Vector3(0, 0, 1)));
        CHECK(options.goals.size() == 3 && bioik_goal_param_count(21) == -1 && BIOIK_MAX_LINK_CAPSULES == 64);
    }
    int hits = 0;
    double worst_device = 0;
    {
        SelfClearanceGoal goal(RW, UA, 0.02, 1.5);
        const double w = against_device(rm, goal, bioik_goal_desc{BIOIK_GOAL_SELF_CLEARANCE, rm.linkIndex(RW), -1, 0, 1.5}, rm.linkIndex(UA), {0.02}, {}, hits);
        std::printf("SelfClearanceGoal with capsules: %d of 100 configurations penetrate, worst relative difference %.3g\n", hits, w);
        CHECK(w >= 0 && hits > 2 && hits < 100);
        worst_device = std::fmax(worst_device, w);
    }
    {
        std::vector<double> obstacles{0.6, -0.2, 0.8, 0.3, 0.4, -0.5, 1.0, 0.2, 0.7, 0.1, 0.6, 0.25};
        ClearanceGoal goal(RW, 0.01, obstacles, 0.8);
        const double w = against_device(rm, goal, bioik_goal_desc{BIOIK_GOAL_CLEARANCE, rm.linkIndex(RW), -1, 0, 0.8}, -1, {0.01}, obstacles, hits);
        std::printf("ClearanceGoal with a capsule: %d of 100 configurations penetrate, worst relative difference %.3g\n", hits, w);
        CHECK(w >= 0 && hits > 2 && hits < 100);
        worst_device = std::fmax(worst_device, w);
    }
    {
        TouchGoal goal(RW, Vector3(0.55, -0.2, 0.7), Vector3(0.2, -0.3, 0.9), 0.7);
        const Vector3 nrm = goal.getNormal();
        const double w = against_device(rm, goal, bioik_goal_desc{BIOIK_GOAL_TOUCH, rm.linkIndex(RW), -1, 0, 0.7}, -1, {0.55, -0.2, 0.7, nrm.x(), nrm.y(), nrm.z()}, {}, hits);
        std::printf("TouchGoal with a capsule: worst relative difference %.3g\n", w);
        CHECK(w >= 0 && hits == 100);
        worst_device = std::fmax(worst_device, w);
    }
    std::printf("host evaluate() with capsules: against the device %.3g\n", worst_device);
    CHECK(worst_device < 1e-13);

    // one query through the plugin core: the default PoseGoal on the wrist, the caller's SelfClearanceGoal between the wrist's capsule and the upper arm's
    using namespace bio_ik_kinematics_plugin;
    BioIKKinematicsPlugin plugin;
    BioIKParams bp;
    bp.gpu_population = 64, bp.gpu_max_steps = 48, bp.random_seed = 3, bp.gpu_islands = 4;
    CHECK(plugin.initialize(rm, "right_arm", "base_footprint", {RW}, 0.0, bp));
    std::vector<double> target = rm.defaultPositions(), bent = rm.defaultPositions();
    const double at[7] = {0.33, 0.09, -3.74, -0.79, -0.5, -1.31, -2.54};   // (the elbow a quarter bent: the hand well outside the upper arm's capsule)
    const double from[7] = {0.1, 0.3, -3.0, -2.3, -0.5, -1.0, -2.0};       // (the elbow bent as far as it goes: the hand inside it)
    size_t k = 0;
    for (const std::string& jn : plugin.getJointNames()) target[rm.joint_first_variable[rm.jointIndex(jn)]] = at[k], bent[rm.joint_first_variable[rm.jointIndex(jn)]] = from[k], k++;
    HostGoalProblem::Model hm;
    for (size_t v = 0; v < rm.variable_names.size(); v++) hm.info.addVariable(rm.var_min[v], rm.var_max[v], rm.var_bounded[v] != 0, rm.var_max_velocity[v], true, false);
    hm.variable_index = [&](const std::string& s) { return rm.variableIndex(s); };
    hm.link_frame = [&](const std::string& s, const std::vector<double>& p) {
        double f[7];
        rm.linkTransform(rm.linkIndex(s), p, f);
        return Frame(Vector3(f[0], f[1], f[2]), Quaternion(f[3], f[4], f[5], f[6]));
    };
    hm.link_points = [&](const std::string& s) { return rm.collisionPoints(s); };
    hm.link_capsules = [&](const std::string& s) { return rm.collisionCapsules(s); };
    std::vector<int> active;
    for (const std::string& jn : plugin.getJointNames()) active.push_back(rm.joint_first_variable[rm.jointIndex(jn)]);
    std::vector<double> seed = rm.defaultPositions();
    SelfClearanceGoal wide(RW, UA, 0.04), asked(RW, UA, 0.02);
    HostGoalProblem clear4(hm, {&wide}, active, seed), clear2(hm, {&asked}, active, seed);
    CHECK(clear4.evaluateGoals(target)[0] == 0.0 && clear2.evaluateGoals(bent)[0] > 1e-4);  // (an answer exists; the start is none)
    double f[7];
    rm.linkTransform(rm.linkIndex(RW), target, f);
    geometry_msgs::Pose pose;
    pose.position.x = f[0], pose.position.y = f[1], pose.position.z = f[2];
    pose.orientation.x = f[3], pose.orientation.y = f[4], pose.orientation.z = f[5], pose.orientation.w = f[6];
    std::vector<double> start(from, from + 7), solution;
    moveit_msgs::MoveItErrorCodes err;
    BioIKKinematicsQueryOptions opt;
    opt.goals.emplace_back(new SelfClearanceGoal(RW, UA, 0.02));
    const bool ok = plugin.searchPositionIK(pose, start, TEST_TIMEOUT, solution, err, opt);
    CHECK(ok);
    std::vector<double> x = rm.defaultPositions();
    size_t i = 0;
    for (const std::string& jn : plugin.getJointNames()) x[rm.joint_first_variable[rm.jointIndex(jn)]] = solution[i++];
    const double cost = clear2.evaluateGoals(x)[0];
    std::printf("solve: ok %d, cost of the answer at the margin %.3g\n", (int)ok, cost);
    CHECK(cost < 1e-10 + 1e-15);  // the success rule, weighted cost < dtwist^2 (problem.cpp:327-334), plus the rounding of this recomputation
    std::printf("ok\n");
    return 0;
}
