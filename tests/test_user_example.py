"""Source compatibility of the goal (cost) plugin interface with user code written for the reference's interface: a MoveIt user program
(tests/cpp/two_hand_lift.inc: both grippers of the PR2 hold a bar and raise it, the head looks at it, secondary goals shape the answer) is
compiled against bio_ik_amd/cpp (+ the stand-in MoveIt / tf headers of bio_ik_amd/cpp/standin) inside the harness tests/cpp/test_user_example.cpp,
and run through the plugin: tf vectors into the goal setters, BioIKKinematicsQueryOptions through RobotState::setFromIK, the solves on the
host simulator of the kernels."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "cpp", "two_hand_lift.inc")


def build_and_run(libdir, libname, tmp_path, max_steps, islands=None):
    cpp = os.path.join(ROOT, "bio_ik_amd", "cpp")
    lib = str(tmp_path / "libbio_ik.so")
    subprocess.run(["make", "-s", "-C", cpp, "SOLVER_DIR=" + libdir, "SOLVER=" + libname, "OUT=" + lib], check=True)
    exe = str(tmp_path / "test_user_example")
    cmd = ["g++", "-std=c++17", "-O1", "-DEXAMPLE_FILE=\"%s\"" % EXAMPLE, "-DEXAMPLE_MAX_STEPS=%d" % max_steps] + (["-DTEST_ISLANDS=%d" % islands] if islands else []) + [
           "-I", cpp, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(cpp, "standin"), os.path.join(ROOT, "tests", "cpp", "test_user_example.cpp"),
           "-L", str(tmp_path), "-lbio_ik", "-Wl,-rpath," + str(tmp_path), "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_two_hand_user_program_compiles_and_runs(hostsim_lib, tmp_path):
    build_and_run(os.path.join(ROOT, "tests", "hostsim"), "bioik_hostsim", tmp_path, max_steps=48, islands=2)
