"""Builds tests/cpp/sessions_test.cpp with g++ alone -- the rule of gx_group_sessions (gorp_amd/csrc/gx_sessions.hpp) is plain C++ --
under AddressSanitizer and UBSan, and runs it as a program of its own: the gap predicate over the corners of int64 (INT64_MIN to
INT64_MAX, equal times, max_gap 0 and INT64_MAX, a difference of exactly max_gap and of max_gap + 1), the head rule, the plan helpers,
and a host replay of the two sorts, the heads and their scan against std::stable_sort and a loop."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_of_sessions_as_a_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sessions_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sessions_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "sessions rule ok" in out.stdout
