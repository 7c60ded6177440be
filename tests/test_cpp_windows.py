"""Builds tests/cpp/windows_test.cpp with g++ alone -- the rule of gx_group_windows (gorp_amd/csrc/gx_windows.hpp) is plain C++ -- under
AddressSanitizer and UBSan, and runs it as a program of its own: the window's predicate over the corners of int64 (INT64_MIN to INT64_MAX
with window INT64_MAX, a difference of exactly the window and of the window + 1, window 0, equal times), the trip rule, the peak word's
tie-break, the 128-bit sum, and a host replay of gallop + bisect against a linear scan, on drawn runs and on runs where the key changes
at e - 1, e - 2, e - 2^k."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_of_windows_as_a_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "windows_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "windows_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "windows rule ok" in out.stdout
