"""The flux B = curl A through the C++ front end on tensor hexahedra (FiniteElementSpace::GetDiscreteInterpolator on a
Raviart-Thomas space with a Nedelec space: the sum-factorised discrete curl of palace_amd/csrc/pa_curl_hex.hip) and
CurlFluxErrorEstimator on the computed flux: examples/cxx_host/flux_hex.cpp against linalg.Curl, the oracle and the estimator
procedure of the Python mirror (tests/test_mixed_hex_gpu.py: device_estimate)."""
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
    d = tmp_path_factory.mktemp("cxx_curl_hex")
    out = str(d / "flux_hex")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "flux_hex.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", out])
    return out, d


@pytest.mark.parametrize("p", [2, 4])
def test_cxx_hex_flux(exe, p):
    import torch

    import dump_estimator_hex_problem as dp
    from palace_amd import linalg
    from tests import curl_util as cu
    from tests import transfer_util as tu
    from tests.test_mixed_hex_gpu import device_estimate

    binary, d = exe
    blob, out = str(d / f"problem{p}.bin"), str(d / f"flux{p}.bin")
    dp.main(blob, p)
    r = subprocess.run([binary, blob, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert re.search(r"refused: .*gradient from the H1 space.*curl from the tensor Nedelec space", r.stdout), r.stdout
    P = dp.problem(p)
    ne, nrt, nnd = P["mesh"].ne, P["rt"].ndofs, P["nd"].ndofs
    got = np.fromfile(out, dtype=np.float64)
    assert got.size == nrt + nnd + ne + nnd
    B, CtB, est, H = np.split(got, [nrt, nrt + nnd, nrt + nnd + ne])
    # the same kernel on the same inputs through the Python mirror, and the oracle
    T = linalg.Curl(linalg.Context(), P["nd"], P["rt"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    B_p = T.mult(dev(P["E"]), torch.empty(nrt, dtype=torch.float64, device="cuda")).cpu().numpy()
    CtB_p = T.mult_transpose(dev(P["B"]), torch.empty(nnd, dtype=torch.float64, device="cuda")).cpu().numpy()
    o = cu.oracle_of(P["nd"], P["rt"], p)
    for name, a, mirror, ref in (("B", B, B_p, o.mult(P["E"])), ("C^T B", CtB, CtB_p, o.mult_transpose(P["B"]))):
        e_m, e_o = tu.rel(a, mirror), tu.rel(a, ref)
        print(f"{name}: against linalg.Curl {e_m:.2e} (max difference {np.abs(a - mirror).max():.2e}), against the oracle {e_o:.2e}")
        assert e_m < 1e-13 and e_o < 1e-13
    est_p, flux_p, its_p = device_estimate(P["mesh"], p, "curl", B, P["muinv"])
    ee, ef = np.abs(est - est_p).max() / est_p.max(), np.abs(H - flux_p).max() / np.abs(flux_p).max()
    its = int(re.search(r"curl: pcg_its (\d+)", r.stdout).group(1))
    print(f"curl: estimates {ee:.2e} smooth flux {ef:.2e} iterations {its} / {its_p}")
    assert ee < 1e-9 and ef < 1e-9 and est_p.min() > 0
    assert abs(its - its_p) <= 1
