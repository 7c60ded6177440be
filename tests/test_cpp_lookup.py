"""Builds tests/cpp/lookup_test.cpp with g++ alone -- the rule of gx_lookup_lines (gorp_amd/csrc/gx_lookup.hpp) is plain C++ -- under
AddressSanitizer and UBSan, and runs it as a program of its own: the find-only probe against find-or-insert on a GroupHostTable with drawn
dictionaries in 64- and 128-slot tables, the weak hash, chains that run past the last slot to slot 0, a miss ended by the first empty
slot, duplicates inserted in every order giving the same entry_same, the empty entry, entries that are prefixes of each other and
entries that differ in the last unit only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_of_lookup_as_a_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lookup_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "gorp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lookup_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert "lookup rule ok" in out.stdout
