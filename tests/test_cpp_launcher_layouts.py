"""The solve launcher's buffer layouts (bio_ik_amd/csrc/bioik_layouts.h: the I/O arena of a host-pointer call, the island scratch, the hand-over workspace) over a grid
of call dimensions, driven by tests/cpp/test_launcher_layouts.cpp: block order, overlap, alignment, the end of the last block, and the total against the closed form the
launcher has always asked for, the sizes of ADVICE.md's finding 1 among them.  A stand-alone host program over the header alone (no library, no device), built and run
twice: plainly, and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_cpp_launcher_layouts(flags, tmp_path):
    exe = str(tmp_path / "test_launcher_layouts")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall"] + flags + ["-I", os.path.join(ROOT, "bio_ik_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_launcher_layouts.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
