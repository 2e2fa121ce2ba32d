"""The host-side plan of the attention launches (csrc/attn_plan.h) on its own: the
stand-alone program tests/cpp/attn_plan_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a child process, sweeps both directions, both head
dims, dropout and keep buffer on and off, head counts around the resident threshold and
every N in 1..700 and asserts that the path equals a literal transcription of the rule, that
each plan names a built kernel or throws in a listed case, that every built kernel is
planned, and the grid, block, LDS and keep-word formulas.  The header is plain C++: no HIP,
no torch, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddim_cold_amd", "csrc")


def test_attn_plan_header_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = tmp_path / "attn_plan_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "attn_plan_check.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stderr + r.stdout)[-4000:]
    assert "checks passed" in r.stdout
