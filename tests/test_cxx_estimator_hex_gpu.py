"""The flux error estimators on tensor-product hexahedra through the C++ front end (palace_amd/csrc/errorestimator.hpp on a
tensor Mesh with a Nedelec and a Raviart-Thomas FiniteElementSpace: BilinearForm(trial, test) reaching pa_op_add_sub_mixed,
FluxErrorEstimatorBase reaching pa_error_op_create_tensor): examples/cxx_host/estimate_hex.cpp against the same procedure through
the Python mirror (tests/test_mixed_hex_gpu.py: device_estimate, itself checked against the oracle there)."""
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


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("cxx_estimator_hex")
    out = str(d / "estimate_hex")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "estimate_hex.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", out])
    return out, d


@pytest.mark.parametrize("p", [2, 4])
def test_cxx_hex_estimators(exe, p):
    import dump_estimator_hex_problem as dp
    from tests.test_mixed_hex_gpu import device_estimate

    binary, d = exe
    blob, out = str(d / f"problem{p}.bin"), str(d / f"est{p}.bin")
    dp.main(blob, p)
    r = subprocess.run([binary, blob, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    P = dp.problem(p)
    ne, nrt, nnd = P["mesh"].ne, P["rt"].ndofs, P["nd"].ndofs
    got = np.fromfile(out, dtype=np.float64)
    assert got.size == 3 * ne + nrt + nnd
    eg, ec, both, D, H = np.split(got, [ne, 2 * ne, 3 * ne, 3 * ne + nrt])
    for name, est, flux, field, mats in (("grad", eg, D, P["E"], P["eps"]), ("curl", ec, H, P["B"], P["muinv"])):
        est_p, flux_p, its_p = device_estimate(P["mesh"], p, name, field, mats)
        ee, ef = np.abs(est - est_p).max() / est_p.max(), np.abs(flux - flux_p).max() / np.abs(flux_p).max()
        its = int(re.search(name + r": pcg_its (\d+)", r.stdout).group(1))
        print(f"{name}: estimates {ee:.2e} smooth flux {ef:.2e} iterations {its} / {its_p}")
        assert ee < 1e-9 and ef < 1e-9 and est_p.min() > 0
        assert abs(its - its_p) <= 1
    # TimeDependentFluxErrorEstimator: the two estimates added, then the square root (Et = 0)
    assert np.abs(both - np.sqrt(eg + ec)).max() < 1e-12 * both.max()
