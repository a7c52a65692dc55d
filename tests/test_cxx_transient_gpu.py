"""The transient driver through the C++ front end (examples/cxx_host/transient.cpp): palace::fem forms with domain and boundary
integrators, KspSolver for M and for A(a), and palace::TimeOperator with the callback that builds A(a) and its solver on the
p-hierarchy -- the reference's coaxial example, 200 steps.  Its printed series (V[1], V[2], E_elec, E_mag) against the same run
through the C ABI (tests/test_transient_gpu.py::test_coaxial_matched_on_the_device) and against the recorded outputs of the
reference."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "cxx_host"))

# The C++ run against the C-ABI run, relative to each column's peak: the gate of the coaxial run in tests/test_transient_gpu.py
# (COAXIAL_GATE).  Both solve every step to the configuration's 1e-8, so what may separate them is the residual each accepts;
# measured on an MI355X they took the same iterations and differ by 2.8e-16 (V[1]), 9.9e-15 (V[2]), 1.9e-15 (E_elec), 2.2e-15
# (E_mag).  No tighter gate is formed from that: two runs of the same device code already differ by 5e-12 in I[1] (summation order
# of the floating-point atomics), and one iteration more or less in one solve moves a series by the size of the tolerance.
GATE = 1e-7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("cxx_transient")
    out = str(d / "transient")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "transient.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", out])
    return out, d


def test_cxx_coaxial_transient(exe):
    import dump_transient_problem as dp

    from palace_amd import linalg
    from palace_amd.fem import transient as tr
    from tests import transient_util as tu

    binary, d = exe
    blob = str(d / "coaxial.bin")
    dp.main(blob)
    r = subprocess.run([binary, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-2000:] + r.stderr
    rows = re.findall(r"^step (\d+) t (\S+) V1 (\S+) V2 (\S+) E_elec (\S+) E_mag (\S+)$", r.stdout, re.M)
    assert [int(x[0]) for x in rows] == list(range(201))
    got = {k: np.array([float(x[i]) for x in rows]) for i, k in ((2, "V1"), (3, "V2"), (4, "E_elec"), (5, "E_mag"))}
    st = dict(re.findall(r"(\w+) (\d+)", r.stdout[r.stdout.index("stats:"):]))
    n = 200
    assert (int(st["steps"]), int(st["k"]), int(st["c"]), int(st["curl"]), int(st["a_solves"]), int(st["m_solves"])) == (n, n + 1, n + 1, n + 1, n, 1)
    assert int(st["ew"]) == 3 + 4 * n
    # the callback ran once (dt never changes), built the solver the class then reports, and every solve went through it
    assert (int(st["configures"]), int(st["rebuilds"]), int(st["same_solver"]), int(st["ksp_mult"])) == (1, 1, 1, n)
    assert int(st["ksp_its"]) > n and "Time stepping: 200 steps" in r.stdout  # (PrintStats)

    system = tr.TransientReferenceSystem(linalg.Context(), tu.coaxial_mesh())
    system.build_device()
    ref = system.run_device()
    times = np.array([float(x[1]) for x in rows]) * system.tc_ns
    assert np.abs(times - ref["t_ns"]).max() <= 1e-12
    gold = tu.golden()
    for k in got:
        dev = np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()
        print(f"C++ against the C-ABI run {k}: {dev:.2e}")
        assert dev <= GATE, (k, dev)
        assert tr.regression_close(got[k], gold[k]).all(), k
        assert np.abs(got[k] - gold[k]).max() <= 2.0e-2 * np.abs(gold[k]).max()
