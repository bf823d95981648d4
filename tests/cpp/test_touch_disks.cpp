// C++ driver of bio_ik::TouchGoal on cylinders and cones, tests/test_cpp_touch_disks.py.
// Default build: bio_ik/urdf.h records the <cylinder> of the link named by argv[2] as a solid and leaves its marker row; RobotModel::resolveCollisionSolids()
// turns it into its two end disks (printed for the comparison with the Python reader); the host evaluation agrees with the goal's formula written out here by
// rotation matrix; and -- with "solve" as the third argument -- one query is solved through the plugin core.
// With -DTEST_MOVEIT_TABLES: the MoveIt plugin's translation unit is compiled into this program against the stand-in MoveIt headers, and its table builder
// (FlatModel) is fed a shapes::Cylinder, a shapes::Cone and a shape it cannot convert.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <vector>

#ifdef TEST_MOVEIT_TABLES
#include "../../bio_ik_amd/cpp/src/kinematics_plugin_hip.cpp"

static bool near(double a, double b) { return std::fabs(a - b) <= 4e-16; }

int main() {
    using bio_ik_kinematics_plugin::FlatModel;
    moveit::core::RobotModel rm;
    rm.addLink("base", "", "root_joint", "fixed", 0, 0, 0, 0, 0, 0, 0, 0, 1);
    rm.addLink("rod", "base", "j1", "revolute", 0.1, 0, 0, 0, 0, 0, 0, 0, 1, -1.0, 1.0, 1.0);
    rm.addLink("tip", "rod", "j2", "revolute", 0.1, 0, 0, 0, 0, 0, 0, 1, 0, -1.0, 1.0, 1.0);
    rm.addLink("odd", "tip", "j3", "fixed", 0, 0, 0, 0, 0, 0, 0, 0, 1);
    // a quarter turn about x (z -> -y) and a shift, on both shapes
    Eigen::Isometry3d o = Eigen::Isometry3d::Identity();
    o.linear()(1, 1) = 0, o.linear()(1, 2) = -1, o.linear()(2, 1) = 1, o.linear()(2, 2) = 0;  // (element access only: real Eigen and the stand-in both have it)
    o.translation() = Eigen::Vector3d(0.5, 0.0, -0.25);
    rm.addShape("rod", shapes::ShapeConstPtr(new shapes::Cylinder(0.03, 0.2)), o);
    rm.addShape("tip", shapes::ShapeConstPtr(new shapes::Box(0.2, 0.4, 0.6)), Eigen::Isometry3d::Identity());
    rm.addShape("tip", shapes::ShapeConstPtr(new shapes::Cone(0.04, 0.1)), o);
    rm.addShape("odd", shapes::ShapeConstPtr(new shapes::Cylinder(0.01, 0.1)), Eigen::Isometry3d::Identity());
    rm.addShape("odd", shapes::ShapeConstPtr(new shapes::Shape()), Eigen::Isometry3d::Identity());  // no convertible kind: the marker, and only for it
    FlatModel fm(rm);
    const bioik_model_desc d = fm.desc();
    const int32_t want_disk_first[5] = {0, 0, 2, 3, 5}, want_point_first[5] = {0, 0, 0, 9, 10};
    for (int l = 0; l < 5; l++)
        if (!d.link_disk_first || !d.link_point_first || d.link_disk_first[l] != want_disk_first[l] || d.link_point_first[l] != want_point_first[l]) {
            std::printf("offsets of link %d wrong\n", l);
            return 1;
        }
    const double want_disks[5][8] = {{0.5, 0.1, -0.25, 0.03, 0, -1, 0, 0}, {0.5, -0.1, -0.25, 0.03, 0, -1, 0, 0}, {0.5, 0.05, -0.25, 0.04, 0, -1, 0, 0},
                                     {0, 0, -0.05, 0.01, 0, 0, 1, 0}, {0, 0, 0.05, 0.01, 0, 0, 1, 0}};
    for (int r = 0; r < 5; r++)
        for (int c = 0; c < 8; c++)
            if (!near(d.link_disks[8 * r + c], want_disks[r][c])) {
                std::printf("disk %d column %d: %.17g\n", r, c, d.link_disks[8 * r + c]);
                return 1;
            }
    const double apex[4] = {0.5, -0.05, -0.25, 0.0}, marker[4] = {0, 0, 0, -1};
    for (int c = 0; c < 4; c++)
        if (!near(d.link_points[4 * 8 + c], apex[c]) || d.link_points[4 * 9 + c] != marker[c]) {
            std::printf("apex or marker row wrong\n");
            return 1;
        }
    if (fm.disks_of_link[1].size() != 16 || fm.disks_of_link[2].size() != 8 || fm.points_of_link[2].size() != 36 || fm.points_of_link[1].size() != 0) return 1;
    std::printf("moveit tables ok\n");
    return 0;
}
#else
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

// d = min(min_i (n_l . v_i - r_i), min_j (n_l . c_j - r_j |n_l x a_j|)) - n . (position - p), n_l = R^T n with R the rotation MATRIX of the link's quaternion
static double formula(const double* f, const double* pos, const double* n, const std::vector<double>* pts, const std::vector<double>* disks) {
    const double x = f[3], y = f[4], z = f[5], w = f[6];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    double nl[3];
    for (int c = 0; c < 3; c++) nl[c] = R[0][c] * n[0] + R[1][c] * n[1] + R[2][c] * n[2];
    double m = 1e300;
    if (pts)
        for (size_t i = 0; i + 4 <= pts->size(); i += 4) m = std::fmin(m, nl[0] * (*pts)[i] + nl[1] * (*pts)[i + 1] + nl[2] * (*pts)[i + 2] - (*pts)[i + 3]);
    if (disks)
        for (size_t i = 0; i + 8 <= disks->size(); i += 8) {
            const double* k = disks->data() + i;
            const double cx = nl[1] * k[6] - nl[2] * k[5], cy = nl[2] * k[4] - nl[0] * k[6], cz = nl[0] * k[5] - nl[1] * k[4];
            m = std::fmin(m, nl[0] * k[0] + nl[1] * k[1] + nl[2] * k[2] - k[3] * std::sqrt(cx * cx + cy * cy + cz * cz));
        }
    return m - (n[0] * (pos[0] - f[0]) + n[1] * (pos[1] - f[1]) + n[2] * (pos[2] - f[2]));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    using namespace bio_ik;
    const std::string rod = argv[2];
    std::shared_ptr<RobotModel> m = loadURDF(slurp(argv[1]));
    // as the reader leaves it: the solid recorded, the marker row in its place, no disks
    const int rod_i = m->linkIndex(rod);
    if (m->link_solids[rod_i].size() != 1 || m->link_solids[rod_i][0].kind != "cylinder" || m->collisionDisks(rod) || !m->collisionPoints(rod) ||
        m->collisionPoints(rod)->size() != 4 || (*m->collisionPoints(rod))[3] != -1.0) {
        std::printf("the reader's record of the cylinder is wrong\n");
        return 1;
    }
    std::printf("solid %s %s %.17g %.17g\n", rod.c_str(), m->link_solids[rod_i][0].kind.c_str(), m->link_solids[rod_i][0].radius, m->link_solids[rod_i][0].length);
    m->resolveCollisionSolids(rod);
    if (!m->collisionDisks(rod) || m->collisionDisks(rod)->size() != 16 || !m->collisionPoints(rod)->empty() || !m->link_solids[rod_i].empty()) {
        std::printf("resolveCollisionSolids left the wrong rows\n");
        return 1;
    }
    for (size_t l = 0; l < m->link_names.size(); l++) {
        const std::vector<double>* p = m->collisionDisks(m->link_names[l]);
        std::printf("disks %s", m->link_names[l].c_str());
        if (p)
            for (double v : *p) std::printf(" %.17g", v);
        std::printf("\n");
    }
    const bioik_model_desc d = m->desc();
    std::printf("desc_disk_first");
    for (size_t l = 0; l <= m->link_names.size(); l++) std::printf(" %d", d.link_disk_first ? d.link_disk_first[l] : 0);
    std::printf("\ndesc_point_first");
    for (size_t l = 0; l <= m->link_names.size(); l++) std::printf(" %d", d.link_point_first ? d.link_point_first[l] : 0);
    std::printf("\n");
    // the setters by hand: a cone (MoveIt's: the origin halfway up, the tip on +z) and raw rows
    {
        RobotModel c = *m;
        c.addCollisionCone(rod, 0.04, 0.1);
        c.addCollisionDisks(rod, {1, 2, 3, 0.5, 0, 0.6, 0.8, 0});
        const std::vector<double>& k = *c.collisionDisks(rod);
        const std::vector<double>& p = *c.collisionPoints(rod);
        if (k.size() != 32 || k[16 + 2] != -0.05 || k[16 + 3] != 0.04 || k[16 + 6] != 1.0 || k[24 + 3] != 0.5 || p.size() != 4 || p[2] != 0.05 || p[3] != 0.0) return 1;
        bool threw = false;
        try {
            c.addCollisionDisks(rod, {0, 0, 0, 0.1, 0, 0, 1.1, 0});
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) return 1;
    }
    // the host evaluation (bio_ik/goal_eval.h, what the hybrid path scores with) against the formula
    TouchGoal* touch = new TouchGoal(rod, bio_ik::Vector3(0.1, 0.2, 0.3), bio_ik::Vector3(0, 3, 4), 0.5);
    BioIKKinematicsQueryOptions options;
    options.goals.emplace_back(touch);
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
        hm.link_disks = [rm](const std::string& link) { return rm->collisionDisks(link); };
        std::vector<int> active;
        for (size_t v = 0; v < m->variable_names.size(); v++) active.push_back((int)v);
        std::vector<double> x = m->defaultPositions();
        const std::vector<const Goal*> goal_list{touch};
        HostGoalProblem hp(hm, goal_list, active, x);
        double worst = 0;
        for (int k = 0; k < 20; k++) {
            for (size_t v = 0; v < x.size(); v++) x[v] = m->var_min[v] + (m->var_max[v] - m->var_min[v]) * std::fmod(0.37 * (k + 1) * (v + 2), 1.0);
            double f[7];
            m->linkTransform(rod_i, x, f);
            const double pos[3] = {0.1, 0.2, 0.3}, n[3] = {0, 0.6, 0.8};
            const double dd = formula(f, pos, n, m->collisionPoints(rod), m->collisionDisks(rod));
            const double got = hp.evaluateGoals(x)[0];
            worst = std::fmax(worst, std::fabs(got - dd * dd));
        }
        std::printf("host_eval_error %.3g\n", worst);
        if (!(worst < 1e-13)) return 1;
    }
    if (argc > 3 && std::string(argv[3]) == "solve") {  // one query through the plugin core: the plane through the rod's lowest rim point at a reachable configuration
        using namespace bio_ik_kinematics_plugin;
        BioIKKinematicsPlugin plugin;
        BioIKParams params;
        params.gpu_population = 32, params.gpu_max_steps = 64, params.random_seed = 2, params.gpu_islands = 4;
        m->addChainGroup("arm", m->link_names[0], rod);
        if (!plugin.initialize(*m, "arm", m->link_names[0], {rod}, 0.0, params)) {
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
        m->linkTransform(rod_i, target, f);
        const double n[3] = {0.48, -0.6, 0.64}, zero[3] = {0, 0, 0};
        const double d0 = formula(f, zero, n, m->collisionPoints(rod), m->collisionDisks(rod));  // d(position) = d(0) - n . position: the plane touches with position = d0 n
        BioIKKinematicsQueryOptions opt;
        opt.replace = true;
        opt.goals.emplace_back(new TouchGoal(rod, bio_ik::Vector3(d0 * n[0], d0 * n[1], d0 * n[2]), bio_ik::Vector3(n[0], n[1], n[2])));
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
        m->linkTransform(rod_i, reached, f);
        const double pos[3] = {d0 * n[0], d0 * n[1], d0 * n[2]};
        const double dist = formula(f, pos, n, m->collisionPoints(rod), m->collisionDisks(rod));
        std::printf("solve touch distance %.3g\n", dist);
        if (!(std::fabs(dist) < 1e-5 + 1e-12)) return 1;  // the success rule, weighted |d| < dtwist (problem.cpp:327-334), plus the rounding of this recomputation
    }
    std::printf("ok\n");
    return 0;
}
#endif
