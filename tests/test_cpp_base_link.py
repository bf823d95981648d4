"""Base links in the C++ mirror (tests/cpp/test_base_link_goal.cpp): the reference-style construction with setBaseLinkName compiles, the host evaluate() of the
eleven built-in link goals with a base agrees with the device's cost on 50 configurations, one "tray" query is solved through the plugin core, and a request that
mixes a based goal with a LinkFunctionGoal goes through the hybrid path (host simulator in the CPU suite, the HIP library on a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(libdir, libname, tmp_path, timeout_s=None):
    exe = str(tmp_path / "test_base_link_goal")
    cpp = os.path.join(ROOT, "bio_ik_amd", "cpp")
    cmd = ["g++", "-std=c++17", "-O1"] + (["-DTEST_TIMEOUT=%g" % timeout_s] if timeout_s else []) + [
        "-I", cpp, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_base_link_goal.cpp"),
        "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    worst = re.search(r"50 configurations x 12 goals: worst relative difference (\S+)", r.stdout)
    assert worst and float(worst.group(1)) < 1e-10
    assert "tray relative position error" in r.stdout and "hybrid relative position error" in r.stdout


def test_cpp_base_link_goal(hostsim_lib, tmp_path):
    run(build(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, timeout_s=600.0))


@pytest.mark.gpu
def test_cpp_base_link_goal_on_gpu(tmp_path):
    run(build(os.path.join(ROOT, "bio_ik_amd"), "bioik_hip", tmp_path))
