"""The flux error estimators for a complex field through the C++ front end (ComplexGradFluxErrorEstimator,
ComplexCurlFluxErrorEstimator of palace_amd/csrc/errorestimator.hpp on a tensor Mesh): examples/cxx_host/estimate_hex_complex.cpp
against the same procedure through the Python mirror (tests/test_two_part_hex_gpu.py: complex_device_estimate, itself checked
against the oracle there)."""
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
    assert os.path.exists(hipcc), "no hipcc"
    d = tmp_path_factory.mktemp("cxx_complex_estimator_hex")
    out = str(d / "estimate_hex_complex")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cxx_host", "estimate_hex_complex.cpp"), "-L" + libdir, "-lpalace_amd",
                           "-Wl,-rpath," + libdir, "-o", out])
    return out, d


@pytest.mark.parametrize("p", [2, 4])
def test_cxx_complex_hex_estimators(exe, p):
    import dump_estimator_hex_complex_problem as dp
    from tests.test_two_part_hex_gpu import ERROR2, MIXED2, RT2, complex_device_estimate

    binary, d = exe
    blob, out = str(d / f"problem{p}.bin"), str(d / f"est{p}.bin")
    dp.main(blob, p)
    r = subprocess.run([binary, blob, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    P = dp.problem(p)
    ne, nrt, nnd = P["mesh"].ne, P["rt"].ndofs, P["nd"].ndofs
    got = np.fromfile(out, dtype=np.float64)
    assert got.size == 2 * ne + 2 * nrt + 2 * nnd
    eg, ec, Dr, Di, Hr, Hi = np.split(got, np.cumsum([ne, ne, nrt, nrt, nnd]))
    pair = (p, p + 1)
    for name, est, flux, field, mats in (("grad", eg, (Dr, Di), (P["E"], P["E_im"]), P["eps"]),
                                         ("curl", ec, (Hr, Hi), (P["B"], P["B_im"]), P["muinv"])):
        est_p, flux_p, its_p = complex_device_estimate(P["mesh"], p, name, field[0], field[1], mats)
        ee = np.abs(est - est_p).max() / est_p.max()
        ef = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(flux, flux_p))
        m = re.search(name + r": pcg_its (\d+) checksum (\S+) one_pass flux (\d) mass (\d) error (\d) mass_one_pass_applies (\d+)",
                      r.stdout)
        its = int(m.group(1))
        print(f"{name}: estimates {ee:.2e} smooth flux {ef:.2e} iterations {its} / {its_p}")
        assert ee < 1e-9 and ef < 1e-9 and est_p.min() > 0
        assert abs(its - its_p) <= 1
        assert abs(float(m.group(2)) - est.sum()) < 1e-12 * est.sum()
        # which steps ran one pass over the element data: the flux operator and the error integrator by their lists, the mass
        # of the smooth space by its family (Raviart-Thomas: PA_RT2_CASE; Nedelec: the H(curl) form, at most four points)
        assert int(m.group(3)) == (pair in MIXED2) and int(m.group(5)) == (pair in ERROR2)
        mass_one_pass = (pair in RT2) if name == "grad" else (p + 1 <= 4)
        assert int(m.group(4)) == mass_one_pass
        # ... and the route the PCG took, counted: one two-vector mass apply per iteration where there is such a kernel (the
        # solver may add one for the initial or final residual), none where there is not
        applies = int(m.group(6))
        assert (its <= applies <= its + 2) if mass_one_pass else applies == 0, (applies, its)
    norm = float(re.search(r"indicator: norm (\S+)", r.stdout).group(1))
    # two samples of the running indicator (Et = 0): the root mean square of sqrt(eg) and sqrt(ec)
    assert abs(norm - np.sqrt(((eg + ec) / 2).sum())) < 1e-12 * norm
