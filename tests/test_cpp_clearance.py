"""bio_ik::ClearanceGoal in the C++ mirror (tests/cpp/test_clearance.cpp): the reference-style construction compiles, the host evaluation agrees with the formula and
with the device, one query is solved through the plugin core (host simulator in the CPU suite, the HIP library on a GPU), and a table changed between two calls of
one goal structure takes effect."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(libdir, libname, tmp_path, timeout_s=None):
    exe = str(tmp_path / "test_clearance")
    cpp = os.path.join(ROOT, "bio_ik_amd", "cpp")
    cmd = ["g++", "-std=c++17", "-O1"] + (["-DTEST_TIMEOUT=%g" % timeout_s] if timeout_s else []) + [
        "-I", cpp, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_clearance.cpp"),
        "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_cpp_clearance(hostsim_lib, tmp_path):
    run(build(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, timeout_s=600.0))


@pytest.mark.gpu
def test_cpp_clearance_on_gpu(tmp_path):
    run(build(os.path.join(ROOT, "bio_ik_amd"), "bioik_hip", tmp_path))
