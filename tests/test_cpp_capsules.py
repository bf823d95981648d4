"""Capsules in the C++ mirror (tests/cpp/test_capsules.cpp): the reference-style construction compiles, the host evaluation of ClearanceGoal, SelfClearanceGoal and
TouchGoal with capsules agrees with the device (the difference is printed), and one query is solved through the plugin core on a model built with addCollisionCapsule
(host simulator in the CPU suite, the HIP library on a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(libdir, libname, tmp_path, timeout_s=None):
    exe = str(tmp_path / "test_capsules")
    cpp = os.path.join(ROOT, "bio_ik_amd", "cpp")
    cmd = ["g++", "-std=c++17", "-O1"] + (["-DTEST_TIMEOUT=%g" % timeout_s] if timeout_s else []) + [
        "-I", cpp, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_capsules.cpp"),
        "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert re.search(r"against the device (\S+)", r.stdout) and float(re.search(r"against the device (\S+)", r.stdout).group(1)) < 1e-13


def test_cpp_capsules(hostsim_lib, tmp_path):
    run(build(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, timeout_s=600.0))


@pytest.mark.gpu
def test_cpp_capsules_on_gpu(tmp_path):
    run(build(os.path.join(ROOT, "bio_ik_amd"), "bioik_hip", tmp_path))
