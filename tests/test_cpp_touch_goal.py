"""bio_ik::TouchGoal in the C++ mirror (tests/cpp/test_touch_goal.cpp): the reference-style construction compiles, bio_ik/urdf.h reads the URDF of
tests/test_touch_goal_api.py to the table the Python reader builds, the host evaluation agrees with the formula, and one query is solved through the
plugin core (host simulator in the CPU suite, the HIP library on a GPU)."""
import os
import subprocess

import numpy as np
import pytest

from bio_ik_amd.urdf import load_urdf
from test_touch_goal_api import URDF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(libdir, libname, tmp_path, timeout_s=None):
    exe = str(tmp_path / "test_touch_goal")
    cpp = os.path.join(ROOT, "bio_ik_amd", "cpp")
    cmd = ["g++", "-std=c++17", "-O1"] + (["-DTEST_TIMEOUT=%g" % timeout_s] if timeout_s else []) + [
        "-I", cpp, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_touch_goal.cpp"),
        "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, tmp_path, *more):
    (tmp_path / "robot.urdf").write_text(URDF)
    r = subprocess.run([exe, str(tmp_path / "robot.urdf"), "pad", *more], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout.strip().split("\n")


def check(lines, solve):
    m = load_urdf(URDF)
    tables = {l.split()[1]: np.array([float(x) for x in l.split()[2:]]).reshape(-1, 4) for l in lines if l.startswith("points ")}
    assert list(tables) == m.link_names
    for name in m.link_names:
        want = m.collision_points(name)
        assert tables[name].shape == want.shape and (want.size == 0 or np.abs(tables[name] - want).max() <= 4 * 2.0 ** -53), name  # (libm and numpy sines)
    mesh = [l.split() for l in lines if l.startswith("mesh ")]
    assert mesh == [["mesh", "pad", "package://finger/pad.stl", "scale", "0.5", "0.5", "2", "resolved", "0"]]
    first = [int(x) for x in [l for l in lines if l.startswith("desc_first")][0].split()[1:]]
    assert first == list(m.arrays()["link_point_first"])  # (the pad's unresolved mesh adds its marker row on both sides)
    assert any(l.startswith("host_eval_error") for l in lines)
    if solve:
        assert any(l.startswith("solve touch distance") for l in lines) and "cylinder refused 1" in lines


def test_cpp_touch_goal(hostsim_lib, tmp_path):
    exe = build(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, timeout_s=600.0)
    check(run(exe, tmp_path, "solve"), True)


@pytest.mark.gpu
def test_cpp_touch_goal_on_gpu(tmp_path):
    exe = build(os.path.join(ROOT, "bio_ik_amd"), "bioik_hip", tmp_path)
    check(run(exe, tmp_path, "solve"), True)
