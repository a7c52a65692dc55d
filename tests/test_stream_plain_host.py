"""The plain element -> dof index of the compact-only streaming H(curl) kernels (palace_amd/csrc/pa_stream_host.hpp:
pack_index_plain, index_dof_plain), checked on the CPU against the run-compressed index and the sorted index it is packed from by a
stand-alone program built with the address and undefined-behaviour sanitizers (tests/cpu/stream_plain_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "stream_plain_check.cpp")
INC = os.path.join(ROOT, "palace_amd", "csrc")


def test_plain_index_against_compressed_index(tmp_path):
    exe = str(tmp_path / "stream_plain_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + INC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
