"""The C++ front end on a mesh with hanging nodes with an assembled level 0: examples/cxx_host/solve_nc_assembled.cpp
(BilinearForm::pa_order_threshold = 2, KspSolver with LinearSolver::BOOMER_AMG on H1 diffusion + mass and LinearSolver::AMS on
ND K + M; the algebraic solvers get P^T A P and the true-dof gradient through the device triple product) against the same
solves through the ctypes mirror: iterations +-1 and checksum 1e-6, as tests/test_cxx_nc_gpu.py does.  The unchanged solve_nc.cpp
(partially assembled level 0) is still refused with `amg`."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "examples", "cxx_host")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("cxx_nc_assembled")
    blob, hblob = str(d / "problem.bin"), str(d / "h1.bin")
    subprocess.check_call([sys.executable, os.path.join(CXX, "dump_nc_problem.py"), blob, "2"])
    subprocess.check_call([sys.executable, os.path.join(CXX, "dump_nc_h1_problem.py"), hblob, "2"])
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    exes = {}
    for name in ("solve_nc_assembled", "solve_nc"):
        exes[name] = str(d / name)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                               "-I" + os.path.join(ROOT, "include"), os.path.join(CXX, name + ".cpp"), "-L" + libdir, "-lpalace_amd",
                               "-Wl,-rpath," + libdir, "-o", exes[name]])
    return exes, blob, hblob


def _mirror(coarse):
    """(true dofs, constrained dofs, iterations, sum(x)) of the same solve through the Python mirror."""
    import torch

    from oracle import palace_oracle as po
    from palace_amd import ceed, linalg
    from tests import nc_util as nu
    from tests import test_nc_coarse_gpu as tc
    from tests import util

    ctx = linalg.Context()
    if coarse == "ams":
        levels = tc.nd_levels(ctx)
        n, it, ok, sx = tc.pmg_solve(ctx, levels, "ams")
        assert ok
        return n, levels[0][-1].n_local - n, it, sx
    spaces = [nu.nc_space("C", "h1", p) for p in (1, 2)]
    geom = ceed.GeomFactorData(spaces[0].mesh, 3)
    c_mass = po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([2.08])], dim=1)
    fine = ceed.diffusionmass_operator(geom, spaces[-1], c_mass.pack(), util.make_ctx("identity")[0].pack())
    local = [fine.coarsen(geom, spaces[0]), fine]
    conf = [linalg.Conforming(ctx, s) for s in spaces]
    A = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE, conforming=c) for op, s, c in zip(local, spaces, conf)]
    P = [linalg.Interp(ctx, spaces[0], spaces[1], conforming=conf[0])]
    ess0 = spaces[0].ess_dofs()
    T0 = A[0].parallel_assemble()
    A0 = linalg.AssembledParOperator(ctx, T0, ess0, linalg.DIAG_ONE)
    B = linalg.gmg(ctx, [A0, A[1]], P, linalg.amg(ctx, T0, ess0), cheby_order=4)
    K = linalg.cg(ctx, A[1], B, rel_tol=1e-10, max_it=400)
    n = spaces[1].n_true
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    b = A[1].mult(ones, torch.empty_like(ones))
    b[torch.from_numpy(spaces[1].ess_dofs().astype(np.int64)).cuda()] = 0.0
    x = K.mult(b, torch.zeros_like(b))
    assert K.stats()["converged"]
    return n, spaces[1].n_local - n, K.stats()["iterations"], float(x.sum())


@pytest.mark.parametrize("coarse", ["amg", "ams"])
def test_cxx_nc_assembled_solve(built, coarse):
    exes, blob, hblob = built
    out = subprocess.check_output([exes["solve_nc_assembled"], blob, hblob, coarse], text=True)
    m = re.search(r"ndofs (\d+)\s+constrained (\d+) .* iterations (\d+)\s+converged (\d)\s+\|b - A x\| / \|b\| (\S+)\s+sum\(x\) (\S+)", out)
    assert m, out
    n, ncon, its, conv = (int(m.group(i)) for i in range(1, 5))
    res, sx = float(m.group(5)), float(m.group(6))
    assert conv == 1 and res < 1e-8 and ncon > 0, out
    n_py, ncon_py, its_py, sx_py = _mirror(coarse)
    print(out.strip(), "| mirror:", n_py, ncon_py, its_py, sx_py)
    assert (n, ncon) == (n_py, ncon_py)
    assert abs(its - its_py) <= 1, (out, its_py)
    assert abs(sx - sx_py) < 1e-6 * abs(sx_py)


def test_partially_assembled_level_0_is_still_refused(built):
    """solve_nc.cpp keeps its partially assembled level 0: BOOMER_AMG there is refused as before."""
    exes, blob, _ = built
    r = subprocess.run([exes["solve_nc"], blob, "amg"], capture_output=True, text=True)
    assert r.returncode == 1 and "hanging-node constraints" in r.stderr and "JACOBI_PCG" in r.stderr, r.stderr
