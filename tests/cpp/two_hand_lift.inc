// User code written against the goal (cost) plugin interface of bio_ik (bio_ik/bio_ik.h), as a MoveIt program would hold it: both
// grippers of the PR2 hold a horizontal bar 0.7 m in front of the robot, wrists rolled against each other, and raise it by a centimetre at
// every call of RobotState::setFromIK; the head keeps looking at the right hand, and three goals shape the answer (joint limits, small
// motions, the torso kept low).  tests/cpp/test_user_example.cpp provides the robot, `robot_state`, `joint_model_group` and the hooks
// EXAMPLE_EXPECT_TIP (the pose a finger tip is asked for) and EXAMPLE_AFTER_IK.
bio_ik::BioIKKinematicsQueryOptions options;
options.replace = true;
options.return_approximate_solution = true;

// finger tips of the left gripper, then of the right one; the bar runs along y, each hand closes on it from the front
const std::vector<std::string> finger_tips = {"l_gripper_l_finger_tip_link", "l_gripper_r_finger_tip_link", "r_gripper_l_finger_tip_link",
                                              "r_gripper_r_finger_tip_link"};
const double hand_y[4] = {0.15, 0.15, -0.15, -0.15};
const double finger_y[4] = {0.025, -0.025, 0.025, -0.025};  // in the gripper's frame
// the gripper points ahead, rolled about an axis a little off its own: the left wrist one way, the right one the other
const tf::Quaternion grip_orientation[4] = {tf::Quaternion(tf::Vector3(1.0, 0.0, 0.3), 0.5), tf::Quaternion(tf::Vector3(1.0, 0.0, 0.3), 0.5),
                                            tf::Quaternion(tf::Vector3(1.0, 0.0, -0.3), -0.5), tf::Quaternion(tf::Vector3(1.0, 0.0, -0.3), -0.5)};
// v rotated by the unit quaternion q: v + 2w (u x v) + 2 u x (u x v), u = (x, y, z)
auto rotate = [](const tf::Quaternion& q, const tf::Vector3& v) {
    auto cross = [](const tf::Vector3& a, const tf::Vector3& b) {
        return tf::Vector3(a.y() * b.z() - a.z() * b.y(), a.z() * b.x() - a.x() * b.z(), a.x() * b.y() - a.y() * b.x());
    };
    const tf::Vector3 u(q.x(), q.y(), q.z()), uv = cross(u, v);
    return v + uv * (2.0 * q.w()) + cross(u, uv) * 2.0;
};
std::vector<bio_ik::PoseGoal*> grip;
for (size_t k = 0; k < finger_tips.size(); k++) {
    auto* g = new bio_ik::PoseGoal();
    g->setLinkName(finger_tips[k]);
    g->setOrientation(grip_orientation[k]);
    options.goals.emplace_back(g);
    grip.push_back(g);
}

auto* gaze = new bio_ik::LookAtGoal();
gaze->setLinkName("sensor_mount_link");
gaze->setAxis(tf::Vector3(1, 0, 0));  // the camera looks along the mount's x axis
options.goals.emplace_back(gaze);

options.goals.emplace_back(new bio_ik::AvoidJointLimitsGoal());
options.goals.emplace_back(new bio_ik::MinimalDisplacementGoal());

auto* keep_torso_low = new bio_ik::PositionGoal();
keep_torso_low->setLinkName("torso_lift_link");
keep_torso_low->setWeight(0.5);
keep_torso_low->setPosition(tf::Vector3(-0.05, 0, 0.95));
options.goals.emplace_back(keep_torso_low);

for (int lift = 0;; lift++) {
    const tf::Vector3 bar(0.7, 0.0, 0.98 + 0.01 * lift);
    for (size_t k = 0; k < grip.size(); k++) {
        const tf::Vector3 tip = bar + tf::Vector3(0.0, hand_y[k], 0.0) + rotate(grip_orientation[k], tf::Vector3(0.0, finger_y[k], 0.0));
        grip[k]->setPosition(tip);
        EXAMPLE_EXPECT_TIP(finger_tips[k], tip, grip_orientation[k])
    }
    gaze->setTarget(grip[3]->getPosition());
    const bool solved = robot_state.setFromIK(joint_model_group, EigenSTL::vector_Affine3d(), std::vector<std::string>(), 0, 0.0,
                                              moveit::core::GroupStateValidityCallbackFn(), options);
    EXAMPLE_AFTER_IK(solved)
}
