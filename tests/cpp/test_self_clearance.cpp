// C++ driver of bio_ik::SelfClearanceGoal (bio_ik/goal_types.h; include/bioik_hip.h: BIOIK_GOAL_SELF_CLEARANCE), tests/test_cpp_self_clearance.py: the reference-style
// construction compiles, the host evaluate() -- which reads both links' frames and both links' points -- is compared against the device's cost and the difference
// printed, and one query is solved through the plugin core: the wrist's spheres keep clear of the upper arm's.
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
    m.addCollisionPoints("r_upper_arm_roll_link", {0.1, 0, 0, 0.2, 0, 0}, {0.2, 0.2});  // (generous spheres: a bent elbow brings the hand inside them)
    m.addCollisionPoints("r_wrist_roll_link", {0.0, 0, 0, 0.08, 0, 0}, {0.045, 0.04});
    return m;
}

int main() {
    using namespace bio_ik;
    RobotModel rm = rightArm();
    const std::string UA = "r_upper_arm_roll_link", RW = "r_wrist_roll_link";
    {  // the reference's usage (goals pushed into BioIKKinematicsQueryOptions): both constructors, the setters, the serialisation
        SelfClearanceGoal empty;
        BioIKKinematicsQueryOptions options;
        options.replace = true;
        auto* g = new SelfClearanceGoal(RW, UA, 0.02, 0.5);
        options.goals.emplace_back(g);
        std::vector<double> par;
        g->gpuParams(par);
        CHECK(g->gpuOpcode() == BIOIK_GOAL_SELF_CLEARANCE && empty.gpuOpcode() == 20 && par.size() == 1 && par[0] == 0.02 && g->getWeight() == 0.5 && !g->isSecondary());
        CHECK(g->gpuLinkName() == RW && g->gpuBaseLinkName() == UA && g->getOtherLinkName() == UA && g->gpuObstacles() == nullptr && empty.gpuBaseLinkName().empty());
        empty.setLinkName(RW), empty.setOtherLinkName(UA), empty.setMargin(0.01);
        CHECK(empty.getBaseLinkName() == UA && empty.getMargin() == 0.01);
        GoalContext ctx;
        g->describe(ctx);  // (adds both links: the hybrid path's host evaluation reads both frames)
    }
    // host evaluate() (bio_ik/goal_eval.h, what the hybrid path scores with) against the device
    bioik_model* model = nullptr;
    bioik_model_desc md = rm.desc();
    CHECK(bioik_model_create(&md, 0, &model) == BIOIK_OK);
    SelfClearanceGoal goal(RW, UA, 0.02, 1.5);
    std::vector<bioik_goal_desc> gd{{BIOIK_GOAL_SELF_CLEARANCE, rm.linkIndex(RW), -1, 0, 1.5}};
    std::vector<int32_t> base{rm.linkIndex(UA)};
    const JointModelGroup& jmg = rm.groups.at("right_arm");
    bioik_problem_desc pd{};
    pd.struct_size = sizeof(pd);
    pd.n_group_joints = (uint32_t)jmg.active_joints.size(), pd.group_joints = jmg.active_joints.data();
    pd.n_goals = 1, pd.goals = gd.data(), pd.goal_base_link = base.data();
    bioik_problem* problem = nullptr;
    CHECK(bioik_problem_create(model, &pd, &problem) == BIOIK_OK);
    CHECK(bioik_problem_obstacle_count(problem, 0) == BIOIK_ERR_INVALID_ARGUMENT);  // (no table: both tables are the model's)
    bioik_problem* refused = nullptr;
    pd.goal_base_link = nullptr;
    CHECK(bioik_problem_create(model, &pd, &refused) == BIOIK_ERR_INVALID_ARGUMENT && refused == nullptr);  // the other link is required
    const int D = bioik_problem_active_variable_count(problem);
    std::vector<int32_t> active(D);
    bioik_problem_active_variables(problem, active.data());
    HostGoalProblem::Model hm;
    for (size_t v = 0; v < rm.variable_names.size(); v++) hm.info.addVariable(rm.var_min[v], rm.var_max[v], rm.var_bounded[v] != 0, rm.var_max_velocity[v], true, false);
    hm.variable_index = [&](const std::string& n) { return rm.variableIndex(n); };
    hm.link_frame = [&](const std::string& n, const std::vector<double>& p) {
        double f[7];
        rm.linkTransform(rm.linkIndex(n), p, f);
        return Frame(Vector3(f[0], f[1], f[2]), Quaternion(f[3], f[4], f[5], f[6]));
    };
    hm.link_points = [&](const std::string& n) { return rm.collisionPoints(n); };
    std::mt19937 rng(5);
    auto limit = [&](int v, bool hi) { return rm.var_bounded[v] ? (hi ? rm.var_max[v] : rm.var_min[v]) : (hi ? 3.0 : -3.0); };
    std::vector<double> seed = rm.defaultPositions();
    HostGoalProblem host(hm, {&goal}, std::vector<int>(active.begin(), active.end()), seed);
    double worst_device = 0;
    int hits = 0;
    const int n = 100;
    for (int k = 0; k < n; k++) {
        std::vector<double> x = seed, genes(D);
        for (int i = 0; i < D; i++) x[active[i]] = genes[i] = std::uniform_real_distribution<double>(limit(active[i], false), limit(active[i], true))(rng);
        const std::vector<double> e = host.evaluateGoals(x);
        double dev = 0, sec = 0;
        const double par[1] = {0.02};
        CHECK(bioik_eval_fitness(problem, BIOIK_FK_EXACT, 1, seed.data(), par, nullptr, genes.data(), &dev, &sec) == BIOIK_OK);
        const double fit = host.computeGoalFitness(x);
        CHECK(std::fabs(fit - 2.25 * e[0]) <= 1e-15 * (1 + fit));
        worst_device = std::fmax(worst_device, std::fabs(fit - dev));
        hits += fit > 0;
    }
    std::printf("host evaluate(): %d of %d configurations penetrate; against the device %.3g\n", hits, n, worst_device);
    CHECK(hits > 2 && hits < n && worst_device < 1e-13);
    bioik_problem_destroy(problem);
    bioik_model_destroy(model);

    // one query through the plugin core: the default PoseGoal on the wrist, the caller's SelfClearanceGoal between wrist and upper arm
    using namespace bio_ik_kinematics_plugin;
    BioIKKinematicsPlugin plugin;
    BioIKParams bp;
    bp.gpu_population = 64, bp.gpu_max_steps = 48, bp.random_seed = 3, bp.gpu_islands = 4;
    CHECK(plugin.initialize(rm, "right_arm", "base_footprint", {RW}, 0.0, bp));
    std::vector<double> target = rm.defaultPositions(), bent = rm.defaultPositions();
    const double at[7] = {0.33, 0.09, -3.74, -0.79, -0.5, -1.31, -2.54};   // (the elbow a quarter bent: the hand well outside the upper arm's spheres)
    const double from[7] = {0.1, 0.3, -3.0, -2.3, -0.5, -1.0, -2.0};       // (the elbow bent as far as it goes: the hand inside them)
    size_t k = 0;
    for (const std::string& jn : plugin.getJointNames()) target[rm.joint_first_variable[rm.jointIndex(jn)]] = at[k], bent[rm.joint_first_variable[rm.jointIndex(jn)]] = from[k], k++;
    SelfClearanceGoal wide(RW, UA, 0.04), asked(RW, UA, 0.02);
    HostGoalProblem clear4(hm, {&wide}, std::vector<int>(active.begin(), active.end()), seed), clear2(hm, {&asked}, std::vector<int>(active.begin(), active.end()), seed);
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
