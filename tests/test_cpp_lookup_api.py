"""Builds and runs tests/cpp/lookup_api_test.cpp against include/gorp.hpp + libgorp_hip.so: lookupLines and textLookupLines of the C++
mirror (refusals in their order).  Host-only mode on CPU; the -m gpu variant runs them on the device."""
import os
import subprocess

import pytest

from gorp_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "lookup_api_test")
    rt = N._load_hip_runtime()._name  # the HIP runtime the Python side would use
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lookup_api_test.cpp"),
           "-o", exe, N.LIB_PATH, rt, "-Wl,-rpath," + os.path.dirname(N.LIB_PATH), "-Wl,-rpath," + os.path.dirname(rt),
           "-Wl,--allow-shlib-undefined"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_lookup_api_host_only(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host-only checks ok" in out.stdout


@pytest.mark.gpu
def test_cpp_lookup_api_on_gpu(tmp_path):
    out = subprocess.run([build(tmp_path), "--gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "GPU checks ok" in out.stdout
