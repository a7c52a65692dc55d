"""Raviart-Thomas hexahedra through the C++ front end (palace_amd/csrc/fem.hpp: a tensor FiniteElementSpace of type PA_FE_HDIV,
VectorFEMassIntegrator and DivDivMassIntegrator reaching the sum-factorised kernel, KspSolver with PCG + Jacobi on the mass):
examples/cxx_host/rt_mass_hex.cpp against the oracle and against the same solve through the Python mirror."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples", "cxx_host"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("cxx_rt_hex")
    out = str(d / "rt_mass_hex")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "rt_mass_hex.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", out])
    return out, d


@pytest.mark.parametrize("p", [2, 3])
def test_cxx_rt_hex_forms_and_solve(exe, p):
    import torch

    import dump_rt_hex_problem as dp
    from palace_amd import ceed, linalg
    from palace_amd.fem import rthex
    from palace_amd.fem.basis1d import gauss_legendre

    binary, d = exe
    blob, out = str(d / f"problem{p}.bin"), str(d / f"y{p}.bin")
    dp.main(blob, p)
    r = subprocess.run([binary, blob, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout and "symmetric 1" in r.stdout and "converged 1" in r.stdout, r.stdout + r.stderr
    assert "prolongation refused" in r.stdout and "Raviart-Thomas space has no multigrid hierarchy" in r.stdout, r.stdout
    P = dp.problem(p)
    mesh, sp, q1d = P["mesh"], P["rt"], P["q1d"]
    n = sp.ndofs
    og = util.oracle_geom(mesh, q1d)
    rint, rdiv = rthex.rt_hex_tables(p, gauss_legendre(q1d)[0])
    _, wts = po.hex_quadrature(q1d)
    ceps = po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[np.asarray(a) for a in P["eps"]], dim=3)
    clam = po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[np.array([v]) for v in P["lam"]], dim=1)
    args = (n, sp.elem_dof_lex, sp.elem_sign_lex < 0)
    M = po.CeedOperatorOracle(*args, rint, rint, og, po.QF_HDIV, ceps)
    K = po.CeedOperatorOracle(*args, rint, rdiv, og, po.QF_L2MASS, ceps, clam, qw=wts, deriv_comps=1)
    got = np.fromfile(out, dtype=np.float64).reshape(4, n)
    for row, o in ((0, M), (2, K)):
        y_ref, d_ref = o.apply_add(P["x"], np.zeros(n)), o.diagonal()
        assert np.abs(got[row] - y_ref).max() < 1e-12 * np.abs(y_ref).max()
        assert np.abs(got[row + 1] - d_ref).max() < 1e-12 * np.abs(d_ref).max()
    # the divergence term matters
    assert np.abs(got[2] - got[0]).max() > 1e-3 * np.abs(got[0]).max()
    # the same solve through the Python mirror
    ctx = linalg.Context()
    Mp = linalg.ParOperator(ctx, ceed.rtmass_operator(ceed.GeomFactorData(mesh, q1d), sp, ceps.pack()), np.zeros(0, dtype=np.int32))
    b = torch.empty(n, dtype=torch.float64, device="cuda")
    sol = torch.zeros_like(b)
    Mp.mult(torch.from_numpy(P["d0"]).cuda(), b)
    solver = linalg.cg(ctx, Mp, linalg.jacobi(ctx, Mp), rel_tol=1e-12, max_it=1000)
    solver.mult(b, sol)
    its = int(re.search(r"iterations (\d+)", r.stdout).group(1))
    err = float(re.search(r"\|d - d0\| / \|d0\| (\S+)", r.stdout).group(1))
    assert err < 1e-9
    assert abs(its - solver.stats()["iterations"]) <= 1
