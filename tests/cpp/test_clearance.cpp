// C++ driver of bio_ik::ClearanceGoal (bio_ik/goal_types.h; include/bioik_hip.h: BIOIK_GOAL_CLEARANCE), tests/test_cpp_clearance.py: the reference-style construction
// compiles, the host evaluate() agrees with the goal's formula written out here by rotation matrix and with the device's cost, one query is solved through the
// plugin core, and a table changed between two calls of the same goal structure takes effect.
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
    m.addCollisionPoints("r_forearm_roll_link", {0.05, 0, 0, 0.15, 0, 0, 0.25, 0, 0}, {0.05, 0.05, 0.05});
    m.addCollisionPoints("r_wrist_roll_link", {0.0, 0, 0, 0.08, 0, 0}, {0.045, 0.04});
    return m;
}

// the formula of include/bioik_hip.h with R the rotation MATRIX of the link's quaternion; also the deepest penetration
static double formula(const double* f, double margin, const std::vector<double>& pts, const std::vector<double>& obs, double* deepest = nullptr) {
    const double x = f[3], y = f[4], z = f[5], w = f[6];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    double sum = 0.0, deep = 0.0;
    for (size_t i = 0; i + 4 <= pts.size(); i += 4) {
        double wp[3];
        for (int c = 0; c < 3; c++) wp[c] = f[c] + R[c][0] * pts[i] + R[c][1] * pts[i + 1] + R[c][2] * pts[i + 2];
        for (size_t j = 0; j + 4 <= obs.size(); j += 4) {
            const double s = (margin + pts[i + 3]) + obs[j + 3];
            const double d = std::sqrt((wp[0] - obs[j]) * (wp[0] - obs[j]) + (wp[1] - obs[j + 1]) * (wp[1] - obs[j + 1]) + (wp[2] - obs[j + 2]) * (wp[2] - obs[j + 2]));
            const double pen = s > 0 ? std::fmax(0.0, s - d) : 0.0;
            sum += pen * pen, deep = std::fmax(deep, pen);
        }
    }
    if (deepest) *deepest = deep;
    return sum;
}

int main() {
    using namespace bio_ik;
    RobotModel rm = rightArm();
    const std::string FA = "r_forearm_roll_link", RW = "r_wrist_roll_link";
    std::vector<double> column;  // a column of spheres in front of the targets
    for (int k = 0; k < 9; k++) column.insert(column.end(), {0.45, -0.25, 0.45 + 0.1 * k, 0.07});
    {  // the reference's usage (goals pushed into BioIKKinematicsQueryOptions): both constructors, the setters, the serialisation
        ClearanceGoal empty;
        BioIKKinematicsQueryOptions options;
        options.replace = true;
        auto* g = new ClearanceGoal(FA, 0.02, column, 0.5);
        options.goals.emplace_back(g);
        std::vector<double> par;
        g->gpuParams(par);
        CHECK(g->gpuOpcode() == BIOIK_GOAL_CLEARANCE && empty.gpuOpcode() == 19 && par.size() == 1 && par[0] == 0.02 && g->getWeight() == 0.5 && g->gpuLinkName() == FA && !g->isSecondary());
        CHECK(g->gpuObstacles() && *g->gpuObstacles() == column && empty.gpuObstacles()->empty() && PositionGoal().gpuObstacles() == nullptr);
        empty.setLinkName(RW), empty.setMargin(0.01), empty.addObstacle(Vector3(1, 2, 3), 0.5);
        CHECK(empty.getObstacles() == std::vector<double>({1, 2, 3, 0.5}) && empty.getMargin() == 0.01);
        bool refused = false;
        try {
            empty.addObstacle(Vector3(0, 0, 0), -1.0);
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        CHECK(refused && empty.getObstacles().size() == 4);
    }
    // host evaluate() (bio_ik/goal_eval.h, what the hybrid path scores with) against the formula and against the device
    bioik_model* model = nullptr;
    bioik_model_desc md = rm.desc();
    CHECK(bioik_model_create(&md, 0, &model) == BIOIK_OK);
    ClearanceGoal forearm(FA, 0.02, column, 0.5), wrist(RW, 0.01, column, 1.5);
    std::vector<bioik_goal_desc> gd{{BIOIK_GOAL_CLEARANCE, rm.linkIndex(FA), -1, 0, 0.5}, {BIOIK_GOAL_CLEARANCE, rm.linkIndex(RW), -1, 0, 1.5}};
    const JointModelGroup& jmg = rm.groups.at("right_arm");
    bioik_problem_desc pd{};
    pd.struct_size = sizeof(pd);
    pd.n_group_joints = (uint32_t)jmg.active_joints.size(), pd.group_joints = jmg.active_joints.data();
    pd.n_goals = 2, pd.goals = gd.data();
    bioik_problem* problem = nullptr;
    CHECK(bioik_problem_create(model, &pd, &problem) == BIOIK_OK);
    CHECK(bioik_problem_obstacle_count(problem, 0) == 0 && bioik_problem_obstacle_count(problem, 1) == 0);
    CHECK(bioik_problem_set_obstacles(problem, 0, column.size() / 4, column.data()) == BIOIK_OK && bioik_problem_set_obstacles(problem, 1, column.size() / 4, column.data()) == BIOIK_OK);
    CHECK(bioik_problem_obstacle_count(problem, 0) == 9 && bioik_problem_set_obstacles(problem, 2, 0, nullptr) == BIOIK_ERR_INVALID_ARGUMENT);
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
    HostGoalProblem host(hm, {&forearm, &wrist}, std::vector<int>(active.begin(), active.end()), seed);
    double worst_formula = 0, worst_device = 0;
    int hits = 0;
    const int n = 100;
    for (int k = 0; k < n; k++) {
        std::vector<double> x = seed, genes(D);
        for (int i = 0; i < D; i++) x[active[i]] = genes[i] = std::uniform_real_distribution<double>(limit(active[i], false), limit(active[i], true))(rng);
        double f[7];
        const std::vector<double> e = host.evaluateGoals(x);
        rm.linkTransform(rm.linkIndex(FA), x, f);
        const double c0 = formula(f, 0.02, *rm.collisionPoints(FA), column);
        rm.linkTransform(rm.linkIndex(RW), x, f);
        const double c1 = formula(f, 0.01, *rm.collisionPoints(RW), column);
        worst_formula = std::fmax(worst_formula, std::fmax(std::fabs(e[0] - c0), std::fabs(e[1] - c1)));
        double dev = 0, sec = 0;
        const double par[2] = {0.02, 0.01};
        CHECK(bioik_eval_fitness(problem, BIOIK_FK_EXACT, 1, seed.data(), par, nullptr, genes.data(), &dev, &sec) == BIOIK_OK);
        const double fit = host.computeGoalFitness(x);
        CHECK(std::fabs(fit - (0.25 * e[0] + 2.25 * e[1])) <= 1e-15 * (1 + fit));
        worst_device = std::fmax(worst_device, std::fabs(fit - dev));
        hits += fit > 0;
    }
    std::printf("host evaluate(): %d of %d configurations penetrate; against the formula %.3g, against the device %.3g\n", hits, n, worst_formula, worst_device);
    CHECK(hits > 5 && hits < n && worst_formula < 1e-13 && worst_device < 1e-13);
    bioik_problem_destroy(problem);
    bioik_model_destroy(model);

    // one query through the plugin core: the default PoseGoal on the wrist, the caller's ClearanceGoals on forearm and wrist
    using namespace bio_ik_kinematics_plugin;
    BioIKKinematicsPlugin plugin;
    BioIKParams bp;
    bp.gpu_population = 64, bp.gpu_max_steps = 48, bp.random_seed = 3, bp.gpu_islands = 4;
    CHECK(plugin.initialize(rm, "right_arm", "base_footprint", {RW}, 0.0, bp));
    std::vector<double> target = rm.defaultPositions();
    const double at[7] = {0.33, 0.09, -3.74, -0.79, -0.5, -1.31, -2.54};  // (clear of the column by 4 cm, the hand behind it; the start, the arm stretched out, passes through it)
    size_t k = 0;
    for (const std::string& jn : plugin.getJointNames()) target[rm.joint_first_variable[rm.jointIndex(jn)]] = at[k++];
    double f[7], deep = 0;
    rm.linkTransform(rm.linkIndex(FA), target, f);
    CHECK(formula(f, 0.04, *rm.collisionPoints(FA), column) == 0.0);  // (the target configuration itself is clear: an answer exists)
    rm.linkTransform(rm.linkIndex(RW), target, f);
    CHECK(formula(f, 0.04, *rm.collisionPoints(RW), column) == 0.0);
    geometry_msgs::Pose pose;
    pose.position.x = f[0], pose.position.y = f[1], pose.position.z = f[2];
    pose.orientation.x = f[3], pose.orientation.y = f[4], pose.orientation.z = f[5], pose.orientation.w = f[6];
    std::vector<double> start, solution;
    for (const std::string& jn : plugin.getJointNames()) start.push_back(rm.defaultPositions()[rm.joint_first_variable[rm.jointIndex(jn)]]);
    moveit_msgs::MoveItErrorCodes err;
    auto ask = [&](const std::vector<double>& table, bool& ok, double& worst_pen, double& fitness) {
        BioIKKinematicsQueryOptions opt;
        opt.goals.emplace_back(new ClearanceGoal(FA, 0.02, table));
        opt.goals.emplace_back(new ClearanceGoal(RW, 0.02, table));
        ok = plugin.searchPositionIK(pose, start, TEST_TIMEOUT, solution, err, opt);
        fitness = opt.solution_fitness;
        worst_pen = 0;
        if (!ok) return;
        std::vector<double> x = rm.defaultPositions();
        size_t i = 0;
        for (const std::string& jn : plugin.getJointNames()) x[rm.joint_first_variable[rm.jointIndex(jn)]] = solution[i++];
        for (const std::string& l : {FA, RW}) {
            double g[7], d = 0;
            rm.linkTransform(rm.linkIndex(l), x, g);
            formula(g, 0.02, *rm.collisionPoints(l), table, &d);
            worst_pen = std::fmax(worst_pen, d);
        }
    };
    bool ok = false;
    double fit = 0;
    ask(column, ok, deep, fit);
    std::printf("solve with the column: ok %d, deepest penetration of the margin %.3g\n", (int)ok, deep);
    CHECK(ok && deep < 1e-5 + 1e-12);  // the success rule, weighted cost < dtwist^2 (problem.cpp:327-334): no pair deeper than dtwist, plus the rounding of this recomputation
    // the same goal structure (the compiled problem comes from the cache) with another table: a ball that swallows the whole workspace -- nothing can succeed;
    // then the column again: the first table is back
    bool ok2 = true, ok3 = false;
    double deep2 = 0, deep3 = 0, fit2 = 0, fit3 = 0;
    ask({0.5, -0.2, 0.8, 5.0}, ok2, deep2, fit2);
    std::printf("solve inside a ball of 5 m: ok %d\n", (int)ok2);
    CHECK(!ok2);
    ask(column, ok3, deep3, fit3);
    std::printf("solve with the column again: ok %d, deepest penetration of the margin %.3g\n", (int)ok3, deep3);
    CHECK(ok3 && deep3 < 1e-5 + 1e-12);
    std::printf("ok\n");
    return 0;
}
