// C++ driver of bio_ik::TouchGoal (bio_ik/goal_types.h), tests/test_cpp_touch_goal.py: the reference-style construction compiles, bio_ik/urdf.h reads
// <collision> into the link's point table (printed for the comparison with the Python reader), the host evaluation agrees with the goal's formula
// written out here by rotation matrix, and --
// with "solve" as the third argument -- one query is solved through the plugin core.
#include <cstdio>
#include <fstream>
#include <sstream>

#include <bio_ik/kinematics_plugin.h>
#include <bio_ik/urdf.h>

#ifndef TEST_TIMEOUT
#define TEST_TIMEOUT 0.25
#endif

static std::string slurp(const char* path) {
    std::ifstream f(path);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

// d = min_i ((R^T n) . v_i - r_i) - n . (position - p) with R the rotation MATRIX of the link's quaternion
static double formula(const double* f, const double* pos, const double* n, const std::vector<double>& pts) {
    const double x = f[3], y = f[4], z = f[5], w = f[6];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    double nl[3];
    for (int c = 0; c < 3; c++) nl[c] = R[0][c] * n[0] + R[1][c] * n[1] + R[2][c] * n[2];
    double m = 1e300;
    for (size_t i = 0; i + 4 <= pts.size(); i += 4) m = std::fmin(m, nl[0] * pts[i] + nl[1] * pts[i + 1] + nl[2] * pts[i + 2] - pts[i + 3]);
    return m - (n[0] * (pos[0] - f[0]) + n[1] * (pos[1] - f[1]) + n[2] * (pos[2] - f[2]));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    using namespace bio_ik;
    // the reference's usage (README of bio_ik: goals pushed into BioIKKinematicsQueryOptions), both constructors
    TouchGoal empty;
    BioIKKinematicsQueryOptions options;
    options.replace = true;
    auto* touch = new TouchGoal(argv[2], bio_ik::Vector3(0.1, 0.2, 0.3), bio_ik::Vector3(0, 3, 4), 0.5);
    options.goals.emplace_back(touch);
    std::vector<double> par;
    touch->gpuParams(par);
    if (touch->gpuOpcode() != BIOIK_GOAL_TOUCH || empty.gpuOpcode() != 17 || par.size() != 6 || std::fabs(par[4] - 0.6) > 1e-15 || std::fabs(par[5] - 0.8) > 1e-15 || touch->getWeight() != 0.5 ||
        touch->gpuLinkName() != argv[2] || touch->isSecondary()) {
        std::printf("goal class: wrong serialisation\n");
        return 1;
    }
    std::shared_ptr<RobotModel> m = loadURDF(slurp(argv[1]));
    for (size_t l = 0; l < m->link_names.size(); l++) {
        const std::vector<double>* p = m->collisionPoints(m->link_names[l]);
        std::printf("points %s", m->link_names[l].c_str());
        if (p)
            for (double v : *p) std::printf(" %.17g", v);
        std::printf("\n");
        auto mr = m->link_meshes.find((int)l);
        if (mr != m->link_meshes.end())
            for (auto& r : mr->second) std::printf("mesh %s %s scale %.17g %.17g %.17g resolved %d\n", m->link_names[l].c_str(), r.filename.c_str(), r.scale[0], r.scale[1], r.scale[2], (int)r.resolved);
    }
    const bioik_model_desc d = m->desc();
    std::printf("desc_first");
    for (size_t l = 0; l <= m->link_names.size(); l++) std::printf(" %d", d.link_point_first ? d.link_point_first[l] : 0);
    std::printf("\n");
    // the host evaluation (bio_ik/goal_eval.h, what the hybrid path scores with) against the formula, on the link named by argv[2]
    {
        HostGoalProblem::Model hm;
        for (size_t v = 0; v < m->variable_names.size(); v++) hm.info.addVariable(m->var_min[v], m->var_max[v], m->var_bounded[v] != 0, m->var_max_velocity[v], true, false);
        const RobotModel* rm = m.get();
        hm.variable_index = [rm](const std::string& n) { return rm->variableIndex(n); };
        hm.link_frame = [rm](const std::string& link, const std::vector<double>& p) {
            double f[7];
            rm->linkTransform(rm->linkIndex(link), p, f);
            return Frame(Vector3(f[0], f[1], f[2]), Quaternion(f[3], f[4], f[5], f[6]));
        };
        hm.link_points = [rm](const std::string& link) { return rm->collisionPoints(link); };
        std::vector<int> active;
        for (size_t v = 0; v < m->variable_names.size(); v++) active.push_back((int)v);
        std::vector<double> x = m->defaultPositions();
        const std::vector<const Goal*> goal_list{touch};
        HostGoalProblem hp(hm, goal_list, active, x);
        double worst = 0;
        for (int k = 0; k < 20; k++) {
            for (size_t v = 0; v < x.size(); v++) x[v] = m->var_min[v] + (m->var_max[v] - m->var_min[v]) * std::fmod(0.37 * (k + 1) * (v + 2), 1.0);
            double f[7];
            m->linkTransform(m->linkIndex(argv[2]), x, f);
            const double pos[3] = {0.1, 0.2, 0.3}, n[3] = {0, 0.6, 0.8};
            const double dd = formula(f, pos, n, *m->collisionPoints(argv[2]));
            const double got = hp.evaluateGoals(x)[0], fit = hp.computeGoalFitness(x);
            worst = std::fmax(worst, std::fabs(got - dd * dd));
            if (std::fabs(fit - 0.25 * got) > 1e-15 * (1 + got)) return 1;
        }
        std::printf("host_eval_error %.3g\n", worst);
        if (!(worst < 1e-13)) return 1;
    }
    if (argc > 3 && std::string(argv[3]) == "solve") {  // one query through the plugin core: the plane through the pad's lowest corner at a reachable configuration
        using namespace bio_ik_kinematics_plugin;
        BioIKKinematicsPlugin plugin;
        BioIKParams params;
        params.gpu_population = 32, params.gpu_max_steps = 64, params.random_seed = 2, params.gpu_islands = 4;
        // the pad's <mesh> is only named by the URDF: until its vertices are there a TouchGoal on the pad is refused; the caller supplies them (scaled, at the mesh's origin)
        {
            const RobotModel::MeshRef r = m->link_meshes.at(m->linkIndex(argv[2]))[0];
            std::vector<double> v = {0.06, 0.0, 0.0, -0.06, 0.02, 0.0, 0.0, 0.08, 0.005, 0.0, -0.08, 0.0, 0.01, 0.0, 0.025, 0.0, 0.0, -0.025};
            for (size_t i = 0; i < v.size(); i++) v[i] *= r.scale[i % 3];
            m->addCollisionPoints(argv[2], v, {}, r.origin);
            if (!m->meshesResolved(argv[2])) return 1;
        }
        m->addChainGroup("arm", m->link_names[0], argv[2]);
        if (!plugin.initialize(*m, "arm", m->link_names[0], {argv[2]}, 0.0, params)) {
            std::printf("initialize failed\n");
            return 1;
        }
        std::vector<double> target = m->defaultPositions();
        const JointModelGroup& g = m->groups.at("arm");
        for (size_t k = 0; k < g.active_joints.size(); k++) {
            const int v = m->joint_first_variable[g.active_joints[k]];
            target[v] = m->var_min[v] + (m->var_max[v] - m->var_min[v]) * (0.3 + 0.2 * (double)k);
        }
        double f[7];
        m->linkTransform(m->linkIndex(argv[2]), target, f);
        const double n[3] = {0.48, -0.6, 0.64}, zero[3] = {0, 0, 0};
        const std::vector<double>& pts = *m->collisionPoints(argv[2]);
        const double d0 = formula(f, zero, n, pts);  // d(position) = d(0) - n . position: the plane touches with position = d0 n
        BioIKKinematicsQueryOptions opt;
        opt.replace = true;
        opt.goals.emplace_back(new TouchGoal(argv[2], bio_ik::Vector3(d0 * n[0], d0 * n[1], d0 * n[2]), bio_ik::Vector3(n[0], n[1], n[2])));
        std::vector<double> seed, solution;
        for (const std::string& jn : plugin.getJointNames()) seed.push_back(m->defaultPositions()[m->joint_first_variable[m->jointIndex(jn)]]);
        moveit_msgs::MoveItErrorCodes err;
        geometry_msgs::Pose pose;
        if (!plugin.searchPositionIK(pose, seed, TEST_TIMEOUT, solution, err, opt)) {
            std::printf("solve failed (%d)\n", err.val);
            return 1;
        }
        std::vector<double> reached = m->defaultPositions();
        size_t k = 0;
        for (const std::string& jn : plugin.getJointNames()) reached[m->joint_first_variable[m->jointIndex(jn)]] = solution[k++];
        m->linkTransform(m->linkIndex(argv[2]), reached, f);
        const double pos[3] = {d0 * n[0], d0 * n[1], d0 * n[2]};
        const double dist = formula(f, pos, n, pts);
        std::printf("solve touch distance %.3g\n", dist);
        if (!(std::fabs(dist) < 1e-5 + 1e-12)) return 1;  // the success rule, weighted |d| < dtwist (problem.cpp:327-334), plus the rounding of this recomputation
        // a TouchGoal on the link with the cylinder is refused, not approximated
        BioIKKinematicsQueryOptions bad;
        bad.replace = true;
        bad.goals.emplace_back(new TouchGoal("rod", bio_ik::Vector3(0, 0, 0), bio_ik::Vector3(0, 0, 1)));
        m->addChainGroup("to_rod", m->link_names[0], "rod");
        BioIKKinematicsPlugin p2;
        std::vector<double> s2, sol2;
        bool refused = false;
        try {
            if (p2.initialize(*m, "to_rod", m->link_names[0], {"rod"}, 0.0, params)) {
                for (const std::string& jn : p2.getJointNames()) s2.push_back(0.0);
                refused = !p2.searchPositionIK(pose, s2, TEST_TIMEOUT, sol2, err, bad);
            }
        } catch (const std::exception& e) {
            refused = true;
        }
        std::printf("cylinder refused %d\n", (int)refused);
        if (!refused) return 1;
    }
    std::printf("ok\n");
    return 0;
}
