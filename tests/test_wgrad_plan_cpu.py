"""The host-side plan of ``ops.linear_wgrad_multi`` (csrc/wgrad_plan.h) on its own: the
stand-alone program tests/cpp/wgrad_plan_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a child process, asserts the plan's invariants
over a grid of problem lists, its error cases and the values the project records for its
own workloads.  The header is plain C++: no HIP, no torch, no GPU."""
import os
import shutil
import subprocess

import pytest

from ddim_cold_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddim_cold_amd", "csrc")


def test_wgrad_plan_header_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on the path")
    exe = tmp_path / "wgrad_plan_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "wgrad_plan_check.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "checks passed" in r.stdout


def test_wgrad_embed_slots_follows_the_token_threshold():
    """256-thread workgroups under 16,384 tokens, 512-thread ones from there (part A's count halves)."""
    B, N, D, owners, n_ln, C = 8, 65, 192, 8, 25, 384
    rest = owners * (D // 16) + n_ln * (C // 16)
    assert ops.wgrad_embed_slots(B, N, D, owners, n_ln, C, 16383) == -(-N * D // 256) + rest
    assert ops.wgrad_embed_slots(B, N, D, owners, n_ln, C, 16384) == -(-N * D // 512) + rest
    assert ops.wgrad_embed_slots(B, N, D, owners, 0, C, 520) == -(-N * D // 256) + owners * (D // 16)
