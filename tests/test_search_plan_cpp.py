"""The launch plan of the list-search pass (srrg2_slam_interfaces_amd/csrc/search_plan.h: how many tiles of four, two and one
lane per point a launch of up to four alignments gets so that it fits the workgroups resident together) -- a plain C++ header,
driven by a stand-alone program (tests/cpp/test_search_plan.cpp) built with the address and undefined-behaviour sanitizers:
coverage, capacity, only the last tile partial, no better split of the same workgroups, and the one-lane fallback."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_search_plan.cpp")


def test_search_plan_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    exe = str(tmp_path / "test_search_plan")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    built = subprocess.run([cxx] + flags + san + ["-o", exe, SRC], capture_output=True, text=True)
    if built.returncode != 0:  # (a toolchain without the sanitizer runtimes: the checks themselves still run)
        built = subprocess.run([cxx] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "450 plans PASSED" in out.stdout, out.stdout
