"""The decision line's encode / decode / fits helpers (sentinel_amd/csrc/cluster_line.hpp) on the CPU: a
stand-alone program built with the host compiler under AddressSanitizer and UBSan (tests/host/)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cluster_line_roundtrip_and_fits(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "cluster_line_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sentinel_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "cluster_line_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cluster_line: ok" in r.stdout
