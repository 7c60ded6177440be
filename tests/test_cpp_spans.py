"""Builds tests/cpp/spans_test.cpp with g++ alone -- the rule of gx_group_spans (gorp_amd/csrc/gx_spans.hpp) is plain C++ -- under
AddressSanitizer and UBSan, and runs it as a program of its own: the exact duration over the corners of int64 (INT64_MIN to INT64_MAX
and back, 2^63 and 2^63 - 1 from both ends, equal times), the state rule on every combination of neighbours, and a host replay of the
sort, the heads and their scan against a std::map put / remove loop on random role strings."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_of_spans_as_a_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "spans_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "spans_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "spans rule ok" in out.stdout
