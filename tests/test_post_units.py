"""What the calls on a render's buffers refuse and how their workspaces are laid out (csrc/host/post_check.hpp: the two
denoisers, the temporal accumulation, the adaptive planner, merge and resolve), as a stand-alone program,
tests/post_units.cpp, built with the address and undefined-behaviour sanitizers and run as a child process. What it asserts
is in that file."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(__import__("tests.conftest", fromlist=["has_gpu"]).has_gpu(), reason="sanitizer runs belong on a machine without a GPU")
def test_post_units(tmp_path):
    """The program builds (a build failure is a failure, not a skip), ends with status 0 and leaves no sanitizer report."""
    exe = str(tmp_path / "post_units")
    # (host code only: -x c++ compiles nothing for a device, and -fno-gpu-sanitize says so to whoever reads the line)
    build = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(ROOT, "tests", "post_units.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "post units ok" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
