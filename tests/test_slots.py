"""Builds and runs tests/cpp/slots_test.cpp: LaunchSlots (gorp_amd/csrc/gx_slots.hpp, plain C++) with the test program in the
device's place -- which call reports a broken max_line_bytes promise, in every order two or three batches can meet on a stream,
across the sequence numbers' wrap and on the shared 32nd slot.  No GPU and no HIP: g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_slots_on_the_cpu(tmp_path):
    exe = str(tmp_path / "slots_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gorp_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "slots_test.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "slots checks ok" in out.stdout
