"""The flux error estimators on a hexahedral mesh with hanging nodes through the C++ front end (GradFluxErrorEstimator,
CurlFluxErrorEstimator and their Complex twins of palace_amd/csrc/errorestimator.hpp on spaces that carry a conforming
prolongation): examples/cxx_host/estimate_nc.cpp on mesh C at order 2 against the same procedure through the Python mirror
(tests/test_nc_estimator_gpu.py: NCEstimator, itself checked against the oracle there), with the gate of
tests/test_cxx_estimator_hex_gpu.py."""
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
def run(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    d = tmp_path_factory.mktemp("cxx_estimator_nc")
    exe = str(d / "estimate_nc")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "estimate_nc.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", exe])
    import dump_estimator_nc_problem as dp

    blob, out = str(d / "problem.bin"), str(d / "est.bin")
    dp.main(blob, "C", 2)
    r = subprocess.run([exe, blob, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    P = dp.problem("C", 2)
    ne, nrt, nnd = P["mesh"].ne, P["rt"].n_true, P["nd"].n_true
    got = np.fromfile(out, dtype=np.float64)
    assert got.size == 6 * ne + nrt + nnd
    return P, r.stdout, np.split(got, np.cumsum([ne] * 6 + [nrt]))


def test_cxx_nc_estimators(run):
    """Estimates and smooth fluxes to 1e-9, projector iterations +-1."""
    import torch  # noqa: F401

    from palace_amd import linalg
    from tests.test_nc_estimator_gpu import NCEstimator

    P, stdout, (eg, ec, eg_im, ec_im, eg2, ec2, D, H) = run
    ctx = linalg.Context()
    for name, est, flux, field, mats in (("grad", eg, D, P["E"], P["eps"]), ("curl", ec, H, P["B"], P["muinv"])):
        est_p, flux_p, its_p = NCEstimator(ctx, P["nd"], P["rt"], name, mats).estimate(field)
        ee = np.abs(est - est_p).max() / est_p.max()
        ef = np.abs(flux - flux_p).max() / np.abs(flux_p).max()
        its = int(re.search(r"^" + name + r": pcg_its (\d+)", stdout, re.M).group(1))
        print(f"{name}: estimates {ee:.2e} smooth flux {ef:.2e} iterations {its} / {its_p}")
        assert ee < 1e-9 and ef < 1e-9 and est_p.min() > 0
        assert abs(its - its_p) <= 1


def test_cxx_nc_complex_estimators(run):
    """The complex estimates are the sum of the two real runs (1e-9), and the mass apply inside the PCG took the one-pass route
    P2, Mult2, P^T2 on the constrained space: once per iteration, plus at most two for the first and last residual."""
    P, stdout, (eg, ec, eg_im, ec_im, eg2, ec2, D, H) = run
    for name, both, re_, im_ in (("grad", eg2, eg, eg_im), ("curl", ec2, ec, ec_im)):
        err = np.abs(both - (re_ + im_)).max() / (re_ + im_).max()
        m = re.search(r"complex " + name + r": pcg_its (\d+) one_pass flux (\d) mass (\d) mass_one_pass_applies (\d+)", stdout)
        its, applies = int(m.group(1)), int(m.group(4))
        print(f"{name}: complex against two real runs {err:.2e}, iterations {its}, one-pass mass applies {applies}")
        assert err < 1e-9 and both.min() > 0
        assert int(m.group(3)) == 1 and applies > 0
        assert its <= applies <= its + 2


def test_cxx_nc_refusals(run):
    """use_mg = true on a constrained smooth space is refused with a message that names use_mg = false; use_mg = false on the
    same hierarchy is the Jacobi form, bit for bit."""
    P, stdout, _ = run
    for k in (0, 1):
        m = re.search(r"use_mg %d: refused: (.*)" % k, stdout)
        assert m and "use_mg = false" in m.group(1), stdout
    assert "hierarchy use_mg 0: same 1" in stdout
