"""Ownership types of the library's device memory (palace_amd/csrc/pa_devbuf.hpp), checked on CPU: DevBuf frees every
array exactly once through moves, re-assignment, reset and a set-up that throws half way, release() frees nothing, and the
reference handle deletes at zero (tests/cpu/devbuf_check.cpp, with counting stand-ins for the two device functions)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "devbuf_check.cpp")
INC = os.path.join(ROOT, "palace_amd", "csrc")


def test_devbuf_and_ref_against_counting_stand_ins(tmp_path):
    exe = str(tmp_path / "devbuf_check")
    # plain g++ and no HIP include path: the header reaches the device through two declared functions only
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + INC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
