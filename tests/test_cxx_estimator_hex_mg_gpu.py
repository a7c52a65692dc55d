"""The multigrid (use_mg) option of the flux error estimators through the C++ front end (palace_amd/csrc/errorestimator.hpp:
FluxProjector / ComplexFluxProjector over a FiniteElementSpaceHierarchy; the Raviart-Thomas hierarchy runs on
palace_amd/csrc/pa_prolong_rt_hex.hip): examples/cxx_host/estimate_hex_mg.cpp with hierarchies 1 .. p.  Jacobi and the multigrid
cycle solve the same well-conditioned system to 1e-12, so the estimates agree far below the bound and the cycle needs fewer
iterations."""
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

KINDS = ("grad", "curl", "cgrad", "ccurl")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("cxx_estimator_hex_mg")
    out = str(d / "estimate_hex_mg")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "estimate_hex_mg.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", out])
    return out, d


def _line(stdout, name):
    m = re.search(name + r": levels (\d+) its grad (\d+) curl (\d+) cgrad (\d+) ccurl (\d+) converged (\d) (\d) (\d) (\d) "
                         r"use_mg (\d) (\d) (\d) (\d)", stdout)
    assert m, stdout
    v = [int(g) for g in m.groups()]
    return dict(levels=v[0], its=dict(zip(KINDS, v[1:5])), converged=v[5:9], use_mg=v[9:13])


@pytest.mark.parametrize("p", [2, 3])
def test_cxx_estimators_with_multigrid_projectors(exe, p):
    import dump_estimator_hex_mg_problem as dp

    binary, d = exe
    blob, out = str(d / f"problem{p}.bin"), str(d / f"est{p}.bin")
    dp.main(blob, p)
    r = subprocess.run([binary, blob, out, "1e-12"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    print(r.stdout)
    ne = int(re.search(r"hexes (\d+) order", r.stdout).group(1))
    est = np.fromfile(out, dtype=np.float64).reshape(3, 4, ne)
    jac, mg, amg = _line(r.stdout, "jacobi"), _line(r.stdout, "mg"), _line(r.stdout, "amg")
    # every solve converges; the hierarchy has levels 1 .. p, the other two one level
    assert "all_converged 1" in r.stdout
    for run in (jac, mg, amg):
        assert run["converged"] == [1, 1, 1, 1], run
    assert (jac["levels"], mg["levels"], amg["levels"]) == (1, p, 1)
    assert jac["use_mg"] == [0, 0, 0, 0] and mg["use_mg"] == [1, 1, 1, 1] and amg["use_mg"] == [1, 1, 1, 1]
    # the same estimates with and without use_mg, and on the one-level use_mg path
    assert np.isfinite(est).all() and (est[0] > 0.0).all()
    for k, kind in enumerate(KINDS):
        scale = est[0, k].max()
        d_mg, d_amg = np.abs(est[1, k] - est[0, k]).max() / scale, np.abs(est[2, k] - est[0, k]).max() / scale
        print(f"{kind}: |mg - jacobi| {d_mg:.2e} |amg - jacobi| {d_amg:.2e} of the largest estimate")
        assert d_mg <= 1e-8
        assert d_amg <= 1e-8
    # strictly fewer iterations with the multigrid cycle
    for kind in KINDS:
        assert 0 < mg["its"][kind] < jac["its"][kind], (kind, mg["its"], jac["its"])
    # two Raviart-Thomas levels of equal order are still no hierarchy
    assert "equal-order hierarchy refused" in r.stdout and "Raviart-Thomas space has no multigrid hierarchy" in r.stdout, r.stdout
