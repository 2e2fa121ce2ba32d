"""The host-side plan of the main GEMM family (csrc/gemm_plan.h) on its own: the stand-alone
program tests/cpp/gemm_plan_check.cpp, built with the address and undefined-behaviour
sanitizers and run as a child process, sweeps every family, tile override, split count and
a grid of sizes around every threshold and asserts that each plan names a built kernel or
throws in a listed case, that every built kernel is named by some plan, the documented
fallbacks and the plans the project records for its own launches.  The header is plain
C++: no HIP, no torch, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddim_cold_amd", "csrc")


def test_gemm_plan_header_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = tmp_path / "gemm_plan_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "gemm_plan_check.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "checks passed" in r.stdout
