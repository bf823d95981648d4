"""bio_ik::TouchGoal on cylinders and cones in the C++ mirror (tests/cpp/test_touch_disks.cpp): bio_ik/urdf.h records the cylinder of the URDF of
tests/test_touch_goal_api.py, resolveCollisionSolids() turns it into the disks the Python reader builds, the host evaluation agrees with the formula, one
query is solved through the plugin core (host simulator in the CPU suite, the HIP library on a GPU), and the MoveIt plugin's table builder converts a
stand-in shapes::Cylinder and shapes::Cone."""
import os
import subprocess

import numpy as np
import pytest

from bio_ik_amd.urdf import load_urdf
from test_touch_goal_api import URDF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "bio_ik_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_touch_disks.cpp")


def build(libdir, libname, tmp_path, timeout_s=None, moveit=False):
    exe = str(tmp_path / ("test_touch_disks_moveit" if moveit else "test_touch_disks"))
    flags = ["-DTEST_MOVEIT_TABLES", "-DBIOIK_STANDIN_PLUGINLIB=1", "-I", os.path.join(CPP, "standin")] if moveit else []
    cmd = ["g++", "-std=c++17", "-O1"] + (["-DTEST_TIMEOUT=%g" % timeout_s] if timeout_s else []) + flags + [
        "-I", CPP, "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe, tmp_path, *more):
    (tmp_path / "robot.urdf").write_text(URDF)
    r = subprocess.run([exe, str(tmp_path / "robot.urdf"), "rod", *more], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout.strip().split("\n")


def check(lines):
    m = load_urdf(URDF)
    assert "solid rod cylinder 0.01 0.20000000000000001" in lines
    m.resolve_collision_solids("rod")
    tables = {l.split()[1]: np.array([float(x) for x in l.split()[2:]]).reshape(-1, 8) for l in lines if l.startswith("disks ")}
    assert list(tables) == m.link_names
    for name in m.link_names:
        assert np.array_equal(tables[name], m.collision_disks(name)), name
    k = m.arrays()
    assert [int(x) for x in [l for l in lines if l.startswith("desc_disk_first")][0].split()[1:]] == list(k["link_disk_first"])
    assert [int(x) for x in [l for l in lines if l.startswith("desc_point_first")][0].split()[1:]] == list(k["link_point_first"])
    assert any(l.startswith("host_eval_error") for l in lines) and any(l.startswith("solve touch distance") for l in lines)


def test_cpp_touch_disks(hostsim_lib, tmp_path):
    exe = build(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, timeout_s=600.0)
    check(run(exe, tmp_path, "solve"))


def test_moveit_table_builder(hostsim_lib, tmp_path):
    """(links the simulator only to satisfy the plugin's symbols: the table builder is host code and calls none of them)"""
    exe = build(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, moveit=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("moveit tables ok"), r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_touch_disks_on_gpu(tmp_path):
    exe = build(os.path.join(ROOT, "bio_ik_amd"), "bioik_hip", tmp_path)
    check(run(exe, tmp_path, "solve"))
