// Base links in the C++ mirror (bio_ik/goal_types.h: LinkGoalBase::setBaseLinkName; include/bioik_hip.h: BASE LINKS) on a PR2-like torso with both arms:
// the reference-style construction compiles, describe() names the base link behind the goal's own link, the host evaluate() of every built-in link goal with a
// base agrees with the device's cost, one "tray" query is solved through the plugin core, and a request that mixes a based goal with a LinkFunctionGoal goes
// through the hybrid path, whose host scoring reads the relative frame.
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

static void addArm(bio_ik::RobotModel& m, const std::string& s, double side) {
    const double z[3] = {0, 0, 0}, ax[3] = {1, 0, 0}, ay[3] = {0, 1, 0}, az[3] = {0, 0, 1};
    const double pan_lo = side < 0 ? -2.2854 : -0.7146, pan_hi = side < 0 ? 0.7146 : 2.2854, roll_lo = side < 0 ? -3.9 : -0.8, roll_hi = side < 0 ? 0.8 : 3.9;
    m.addLink(s + "_shoulder_pan_link", "torso_lift_link", s + "_shoulder_pan_joint", "revolute", {0, 0.188 * side, 0}, z, az, pan_lo, pan_hi, 2.088);
    m.addLink(s + "_shoulder_lift_link", s + "_shoulder_pan_link", s + "_shoulder_lift_joint", "revolute", {0.1, 0, 0}, z, ay, -0.5236, 1.3963, 2.082);
    m.addLink(s + "_upper_arm_roll_link", s + "_shoulder_lift_link", s + "_upper_arm_roll_joint", "revolute", z, z, ax, roll_lo, roll_hi, 3.27);
    m.addLink(s + "_elbow_flex_link", s + "_upper_arm_roll_link", s + "_elbow_flex_joint", "revolute", {0.4, 0, 0}, z, ay, -2.3213, 0.0, 3.3);
    m.addLink(s + "_forearm_roll_link", s + "_elbow_flex_link", s + "_forearm_roll_joint", "continuous", z, z, ax, 0, 0, 3.6);
    m.addLink(s + "_wrist_flex_link", s + "_forearm_roll_link", s + "_wrist_flex_joint", "revolute", {0.321, 0, 0}, z, ay, -2.18, 0.0, 3.078);
    m.addLink(s + "_wrist_roll_link", s + "_wrist_flex_link", s + "_wrist_roll_joint", "continuous", z, z, ax, 0, 0, 3.6);
}

static bio_ik::RobotModel twoArms() {
    bio_ik::RobotModel m;
    const double z[3] = {0, 0, 0}, az[3] = {0, 0, 1};
    m.addLink("base_footprint", "", "", "fixed", z, z, az);
    m.addLink("base_link", "base_footprint", "base_footprint_joint", "fixed", {0, 0, 0.051}, z, az);
    m.addLink("torso_lift_link", "base_link", "torso_lift_joint", "prismatic", {-0.05, 0, 0.739675}, z, az, 0.0, 0.33, 0.013);
    addArm(m, "r", -1.0);
    addArm(m, "l", +1.0);
    std::vector<std::string> joints{"torso_lift_joint"};
    for (const char* s : {"r", "l"})
        for (const char* j : {"_shoulder_pan_joint", "_shoulder_lift_joint", "_upper_arm_roll_joint", "_elbow_flex_joint", "_forearm_roll_joint", "_wrist_flex_joint", "_wrist_roll_joint"})
            joints.push_back(std::string(s) + j);
    m.addJointGroup("all", joints, {"r_wrist_roll_link", "l_wrist_roll_link"});
    return m;
}

static bio_ik::Frame linkFrame(const bio_ik::RobotModel& rm, const std::string& n, const std::vector<double>& x) {
    double f[7];
    rm.linkTransform(rm.linkIndex(n), x, f);
    return bio_ik::Frame(bio_ik::Vector3(f[0], f[1], f[2]), bio_ik::Quaternion(f[3], f[4], f[5], f[6]));
}

int main() {
    using namespace bio_ik;
    RobotModel rm = twoArms();
    const std::string RW = "r_wrist_roll_link", LW = "l_wrist_roll_link";
    {  // the reference-style construction: a default-constructed goal and its setters
        auto* g = new PoseGoal();
        g->setLinkName(LW);
        g->setBaseLinkName(RW);
        g->setPosition(Vector3(0.0, 0.4, 0.0));
        g->setOrientation(Quaternion(0, 0, 0, 1));
        BioIKKinematicsQueryOptions opt;
        opt.goals.emplace_back(g);
        CHECK(g->getBaseLinkName() == RW && g->gpuBaseLinkName() == RW && PoseGoal().getBaseLinkName().empty());
    }
    // one of every built-in link goal with the right wrist as its base (host evaluate() against the device), and a world goal beside them
    std::vector<std::unique_ptr<Goal>> goals;
    goals.emplace_back(new PoseGoal(LW, Vector3(0.1, 0.4, -0.1), Quaternion(0.1, 0.2, 0.3, 0.9), 1.0));
    goals.emplace_back(new PositionGoal(LW, Vector3(0.3, -0.3, 0.2), 0.8));
    goals.emplace_back(new OrientationGoal(LW, Quaternion(0.0, 0.3, 0.1, 0.9), 0.6));
    goals.emplace_back(new LookAtGoal(LW, Vector3(1, 0, 0), Vector3(0.2, 0.5, 0.1), 0.5));
    goals.emplace_back(new MaxDistanceGoal(LW, Vector3(0.2, 0.2, 0.2), 0.3, 1.1));
    goals.emplace_back(new MinDistanceGoal(LW, Vector3(0.25, 0.2, 0.5), 0.9, 0.9));
    goals.emplace_back(new LineGoal(LW, Vector3(0.0, 0.0, 0.5), Vector3(0.0, 1.0, 0.5), 0.4));
    goals.emplace_back(new PlaneGoal(LW, Vector3(0.0, 0.0, 0.6), Vector3(0.0, 0.2, 1.0), 0.3));
    goals.emplace_back(new SideGoal(LW, Vector3(0, 0, 1), Vector3(0, 1, 0), 0.7));
    goals.emplace_back(new DirectionGoal(LW, Vector3(0, 0, 1), Vector3(1, 0, 0), 0.2));
    goals.emplace_back(new ConeGoal(LW, Vector3(0.1, 0.0, 0.3), 0.5, Vector3(1, 0, 0), Vector3(0, 0, 1), 0.3, 0.6));
    for (auto& g : goals) static_cast<LinkGoalBase*>(g.get())->setBaseLinkName(RW);
    goals.emplace_back(new PositionGoal(RW, Vector3(0.6, -0.2, 0.8), 0.5));
    CHECK(goals.size() == 12);
    {
        GoalContext c;
        goals[0]->describe(c);
        HostGoalProblem::Model none;
        none.variable_index = [](const std::string&) { return -1; };
        HostGoalProblem names(none, {goals[0].get()}, {}, {});
        CHECK(names.getTipNames().size() == 2 && names.getTipNames()[0] == LW && names.getTipNames()[1] == RW);  // the base link behind the goal's own link
    }
    bioik_model* model = nullptr;
    bioik_model_desc md = rm.desc();
    CHECK(bioik_model_create(&md, 0, &model) == BIOIK_OK);
    std::vector<bioik_goal_desc> gd;
    std::vector<int32_t> base;
    std::vector<double> params;
    for (auto& g : goals) {
        bioik_goal_desc d{g->gpuOpcode(), rm.linkIndex(g->gpuLinkName()), -1, 0, g->getWeight()};
        gd.push_back(d);
        base.push_back(g->gpuBaseLinkName().empty() ? -1 : rm.linkIndex(g->gpuBaseLinkName()));
        g->gpuParams(params);
    }
    const JointModelGroup& jmg = rm.groups.at("all");
    bioik_problem_desc pd{};
    pd.struct_size = sizeof(pd);
    pd.n_group_joints = (uint32_t)jmg.active_joints.size(), pd.group_joints = jmg.active_joints.data();
    pd.n_goals = (uint32_t)gd.size(), pd.goals = gd.data();
    pd.goal_base_link = base.data();
    bioik_problem* problem = nullptr;
    CHECK(bioik_problem_create(model, &pd, &problem) == BIOIK_OK);
    CHECK(bioik_problem_tip_count(problem) == 2 && (size_t)bioik_problem_param_count(problem) == params.size());
    const int D = bioik_problem_active_variable_count(problem);
    CHECK(D == 15);
    std::vector<int32_t> active(D);
    bioik_problem_active_variables(problem, active.data());

    HostGoalProblem::Model hm;
    for (size_t v = 0; v < rm.variable_names.size(); v++) {
        bool revolute = false, prismatic = false;
        for (size_t l = 0; l < rm.joint_type.size(); l++)
            if (rm.joint_first_variable[l] == (int)v) revolute = rm.joint_type[l] == BIOIK_JOINT_REVOLUTE, prismatic = rm.joint_type[l] == BIOIK_JOINT_PRISMATIC;
        hm.info.addVariable(rm.var_min[v], rm.var_max[v], rm.var_bounded[v], rm.var_max_velocity[v], revolute, prismatic);
    }
    hm.variable_index = [&](const std::string& n) { return rm.variableIndex(n); };
    hm.link_frame = [&](const std::string& n, const std::vector<double>& positions) { return linkFrame(rm, n, positions); };
    std::mt19937 rng(11);
    auto uniform = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    auto limit = [&](int v, bool hi) { return rm.var_bounded[v] ? (hi ? rm.var_max[v] : rm.var_min[v]) : (hi ? 3.0 : -3.0); };
    std::vector<double> seed = rm.defaultPositions();
    const int n = 50;
    std::vector<double> genes(n * D), prim(n), sec(n);
    std::vector<std::vector<double>> full(n, seed);
    for (int k = 0; k < n; k++)
        for (int i = 0; i < D; i++) full[k][active[i]] = genes[k * D + i] = uniform(limit(active[i], false), limit(active[i], true));
    double worst = 0.0;
    for (size_t gi = 0; gi < goals.size(); gi++) {  // goal by goal: a problem of its own, so that no cost hides behind a larger one
        bioik_problem_desc one = pd;
        one.n_goals = 1, one.goals = &gd[gi], one.goal_base_link = &base[gi];
        bioik_problem* p1 = nullptr;
        CHECK(bioik_problem_create(model, &one, &p1) == BIOIK_OK);
        const int D1 = bioik_problem_active_variable_count(p1);
        std::vector<int32_t> a1(D1);
        bioik_problem_active_variables(p1, a1.data());
        std::vector<double> g1(n * D1), par;
        goals[gi]->gpuParams(par);
        for (int k = 0; k < n; k++)
            for (int i = 0; i < D1; i++) g1[k * D1 + i] = full[k][a1[i]];
        // (the variables that are not active in this one-goal problem come from the seed: each configuration is its own seed)
        HostGoalProblem host(hm, {goals[gi].get()}, std::vector<int>(a1.begin(), a1.end()), seed);
        for (int k = 0; k < n; k++) {
            double dev = 0, dsec = 0;
            CHECK(bioik_eval_fitness(p1, BIOIK_FK_EXACT, 1, full[k].data(), par.data(), nullptr, &g1[k * D1], &dev, &dsec) == BIOIK_OK);
            const double h = host.computeGoalFitness(full[k], false);
            worst = std::max(worst, std::fabs(h - dev) / std::max(1.0, std::fabs(h)));
        }
        bioik_problem_destroy(p1);
    }
    std::printf("host evaluate() vs device cost with a base link, %d configurations x %zu goals: worst relative difference %.3g\n", n, goals.size(), worst);
    CHECK(worst < 1e-10);
    {  // all twelve in one problem: the sums
        std::vector<const Goal*> ptrs;
        for (auto& g : goals) ptrs.push_back(g.get());
        HostGoalProblem host(hm, ptrs, std::vector<int>(active.begin(), active.end()), seed);
        CHECK(bioik_eval_fitness(problem, BIOIK_FK_EXACT, n, seed.data(), params.data(), nullptr, genes.data(), prim.data(), sec.data()) == BIOIK_OK);
        for (int k = 0; k < n; k++) CHECK(std::fabs(host.computeGoalFitness(full[k], false) - prim[k]) <= 1e-10 * std::max(1.0, prim[k]));
    }
    bioik_problem_destroy(problem);
    bioik_model_destroy(model);

    // "tray" through the plugin core: the plugin's default PoseGoal on the right wrist stays a world goal; the caller's goal poses the left wrist against the right
    using namespace bio_ik_kinematics_plugin;
    BioIKKinematicsPlugin plugin;
    BioIKParams bp;
    bp.gpu_population = 128, bp.gpu_max_steps = 128, bp.random_seed = 2, bp.gpu_islands = 4;
    CHECK(plugin.initialize(rm, "all", "base_footprint", {RW}, 0.0, bp));
    std::vector<double> target = rm.defaultPositions();
    for (int i = 0; i < D; i++) target[active[i]] = limit(active[i], false) + (limit(active[i], true) - limit(active[i], false)) * (0.3 + 0.03 * i);
    const Frame A = linkFrame(rm, RW, target), B = linkFrame(rm, LW, target), R = concat(inverse(A), B);
    geometry_msgs::Pose pose;
    pose.position.x = A.pos.x(), pose.position.y = A.pos.y(), pose.position.z = A.pos.z();
    pose.orientation.x = A.rot.x(), pose.orientation.y = A.rot.y(), pose.orientation.z = A.rot.z(), pose.orientation.w = A.rot.w();
    std::vector<double> start, solution;
    for (const std::string& jn : plugin.getJointNames()) {
        const int v = rm.joint_first_variable[rm.jointIndex(jn)];
        start.push_back(target[v] + 0.05 * (limit(v, true) - limit(v, false)));  // a twentieth of its range away
    }
    auto reachedFrames = [&](const std::vector<double>& sol, Frame& a, Frame& b) {
        std::vector<double> x = rm.defaultPositions();
        size_t k = 0;
        for (const std::string& jn : plugin.getJointNames()) x[rm.joint_first_variable[rm.jointIndex(jn)]] = sol[k++];
        a = linkFrame(rm, RW, x), b = linkFrame(rm, LW, x);
    };
    moveit_msgs::MoveItErrorCodes err;
    {
        BioIKKinematicsQueryOptions opt;
        auto* tray = new PoseGoal(LW, R.pos, R.rot);
        tray->setBaseLinkName(RW);
        opt.goals.emplace_back(tray);
        if (!plugin.searchPositionIK(pose, start, TEST_TIMEOUT, solution, err, opt)) {
            std::printf("tray: solve failed (%d)\n", err.val);
            return 1;
        }
        Frame a, b;
        reachedFrames(solution, a, b);
        const Frame r = concat(inverse(a), b);
        const double dr = r.pos.distance(R.pos), da = a.pos.distance(A.pos);
        std::printf("tray relative position error %.3g world position error %.3g\n", dr, da);
        CHECK(dr < 2e-5 && da < 2e-5);  // (every twist component below dtwist = 1e-5: the position error below sqrt(3) dtwist)
    }
    {  // the hybrid path: a LinkFunctionGoal (no device opcode) beside the based goal; the host scores the candidates with BOTH, the based one on R
        BioIKKinematicsQueryOptions opt;
        auto* tray = new PositionGoal(LW, R.pos);
        tray->setBaseLinkName(RW);
        opt.goals.emplace_back(tray);
        int calls = 0;
        opt.goals.emplace_back(new LinkFunctionGoal(LW, [&calls](const Vector3&, const Quaternion& q) { calls++; return 1e-14 * q.w() * q.w(); }, 1.0));
        opt.return_approximate_solution = true;
        CHECK(plugin.searchPositionIK(pose, start, TEST_TIMEOUT, solution, err, opt));
        CHECK(calls > 0);
        Frame a, b;
        reachedFrames(solution, a, b);
        const double dr = concat(inverse(a), b).pos.distance(R.pos);
        std::printf("hybrid relative position error %.3g (callback evaluated %d times), solution_fitness %.3g\n", dr, calls, opt.solution_fitness);
        // the fitness the plugin reports holds the host's scoring of every goal: with the based goal read in the WORLD frame it would be of the order of |B.p - R.p|^2
        CHECK(opt.solution_fitness < 1e-6 && (B.pos - R.pos).length2() > 1e-2);
    }
    std::printf("ok\n");
    return 0;
}
