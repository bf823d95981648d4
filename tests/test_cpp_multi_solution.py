"""MoveIt's multi-solution getPositionIK of the plugin translation unit (libbio_ik.so, stand-in MoveIt headers), driven through kinematics::KinematicsBase* by
tests/cpp/test_multi_solution.cpp.  CPU suite: linked against the host simulator of the kernels; GPU suite: against libbioik_hip.so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(libdir, libname, tmp_path):
    cpp = os.path.join(ROOT, "bio_ik_amd", "cpp")
    lib = str(tmp_path / "libbio_ik.so")
    subprocess.run(["make", "-s", "-C", cpp, "SOLVER_DIR=" + libdir, "SOLVER=" + libname, "OUT=" + lib], check=True)
    exe = str(tmp_path / "test_multi_solution")
    cmd = ["g++", "-std=c++17", "-O1", "-I", cpp, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(cpp, "standin"),
           os.path.join(ROOT, "tests", "cpp", "test_multi_solution.cpp"), "-L", str(tmp_path), "-lbio_ik", "-Wl,-rpath," + str(tmp_path), "-L", libdir, "-l" + libname,
           "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_multi_solution_on_host_simulator(hostsim_lib, tmp_path):
    build_and_run(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path)


@pytest.mark.gpu
def test_multi_solution_on_gpu(tmp_path):
    build_and_run(os.path.join(ROOT, "bio_ik_amd"), "bioik_hip", tmp_path)
