"""BioIKKinematicsPlugin.searchPositionIKRanked (several solutions per pose, MoveIt's multi-solution getPositionIK in batched form): through the shim over the host
simulator (no GPU) and over the product libraries on the device."""
import numpy as np
import pytest

from bio_ik_amd import BioIKKinematicsPlugin, BioIKKinematicsQueryOptions, JointFunctionGoal, KinematicsQueryOptions
from bio_ik_amd.robot import frame_concat, link_transform
from conftest import random_configuration
from test_plugin import goal_in_base_frame

ARM = ("right_arm", "torso_lift_link", ["r_wrist_roll_link"])


def ranked_checks(pr2, lib, n, islands, steps, k, md):
    params = {"gpu_max_steps": steps, "random_seed": 5, "gpu_reproducible_calls": True, "gpu_islands": islands, "gpu_island_sync": False}
    p = BioIKKinematicsPlugin(lib=lib)
    assert p.initialize(pr2, *ARM, 0.0, params=params)
    rng = np.random.default_rng(22)
    gv = p._group_vars
    targets = np.tile(pr2.default_positions(), (n, 1))
    targets[:, gv] = random_configuration(pr2, rng, n)[:, gv]
    poses = np.stack([goal_in_base_frame(pr2, t) for t in targets]).reshape(n, 1, 7)
    seeds = random_configuration(pr2, rng, n)[:, gv]
    approx = KinematicsQueryOptions(return_approximate_solution=True)
    one, _, _, _ = p.searchPositionIKBatch(poses, seeds, options=approx)
    _, ok1, _, _ = p.searchPositionIKBatch(poses, seeds)  # (the same solve under gpu_reproducible_calls; ok without the approximate ones)
    sols, passed = p.searchPositionIKRanked(poses, seeds, k, md, options=approx)
    lo, hi = np.asarray(pr2.var_min)[gv], np.asarray(pr2.var_max)[gv]
    bounded = np.asarray(pr2.var_bounded)[gv] != 0
    base = link_transform(pr2, pr2.link_index("torso_lift_link"), pr2.default_positions())
    for q in range(n):
        assert 1 <= len(sols[q]) <= k and sols[q].shape[1] == len(gv)
        # row 0 is searchPositionIKBatch's solution with the same explicit island count and the island sync off
        assert np.array_equal(sols[q][0], one[q]) and bool(passed[q][0]) == bool(ok1[q])
        for r, row in enumerate(sols[q]):
            assert np.all(row[bounded] >= lo[bounded]) and np.all(row[bounded] <= hi[bounded])  # bounded like searchPositionIKBatch's
            assert np.all(np.abs(row[~bounded]) <= np.pi + 1e-12) or np.all(np.abs(row - seeds[q])[~bounded] <= np.pi + 1e-12)  # wrapped
            for o in sols[q][:r]:
                assert np.abs(row - o).max() > md
            if passed[q][r]:
                state = pr2.default_positions()
                state[gv] = row
                got = link_transform(pr2, pr2.link_index("r_wrist_roll_link"), state)
                want = frame_concat(base, poses[q, 0])
                assert np.linalg.norm(got[:3] - want[:3]) < 1e-4 and 2 * np.arccos(min(1.0, abs(got[3:] @ want[3:]))) < 1e-3
    # without return_approximate_solution only rows that passed come back
    strict, spassed = p.searchPositionIKRanked(poses, seeds, k, md)
    assert all(bool(np.all(x)) for x in spassed)
    assert [len(x) for x in strict] == [int(np.sum(x)) for x in passed] or all(len(a) <= len(b) for a, b in zip(strict, sols))
    # the yaml keys are the defaults of k and the distance
    p.params["gpu_solutions"], p.params["gpu_solution_distance"] = k, md
    again, _ = p.searchPositionIKRanked(poses, seeds, options=approx)
    assert all(np.array_equal(a, b) for a, b in zip(again, sols))
    # a callback goal is refused
    bio = BioIKKinematicsQueryOptions()
    bio.goals.append(JointFunctionGoal(["r_elbow_flex_joint"], lambda v: v))
    with pytest.raises((NotImplementedError, RuntimeError)):
        p.searchPositionIKRanked(poses, seeds, k, md, options=bio)
    # more solutions than islands can give: refused with a message, not a crash
    with pytest.raises(RuntimeError):
        p.searchPositionIKRanked(poses, seeds, 65, md)
    p.close()
    return sols, passed


def test_ranked_through_the_hostsim_shim(hostsim_shim, pr2):
    ranked_checks(pr2, hostsim_shim, 3, 6, 12, 4, 0.1)


@pytest.mark.gpu
def test_ranked_on_the_device(pr2):
    sols, passed = ranked_checks(pr2, None, 64, 16, 100, 8, 0.1)
    assert sum(int(np.sum(x)) >= 2 for x in passed) >= 1
