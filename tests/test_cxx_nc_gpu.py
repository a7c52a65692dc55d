"""The C++ front end on a mesh with hanging nodes: examples/cxx_host/solve_nc.cpp (FiniteElementSpace carrying the constraint
into BilinearForm::Assemble and FiniteElementSpaceHierarchy, KspSolver with PCG + p-multigrid) on the dump of the reference
cylinder with a seeded quarter of its elements refined, order 2, levels [1, 2], against the same solve through the ctypes
mirror: iterations +-1 and checksum 1e-6, as tests/test_cxx_host_gpu.py does for the conforming case."""
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, "examples", "cxx_host", "dump_nc_problem.py")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("cxx_nc")
    exe, blob = str(d / "solve_nc"), str(d / "problem.bin")
    subprocess.check_call([sys.executable, DUMP, blob, "2"])
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "solve_nc.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", exe])
    return exe, blob


@pytest.fixture(scope="module")
def mirror():
    """The device operators of the same problem through the Python mirror: (ctx, spaces, A per level, P, keep-alive)."""
    from palace_amd import ceed, linalg

    spec = importlib.util.spec_from_file_location("dump_nc_problem", DUMP)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mesh, spaces = mod.problem(2)
    ctx = linalg.Context()
    geom = ceed.GeomFactorData(mesh, 3)
    mass = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[np.array([2.08])])
    fine = ceed.curlcurlmass_operator(geom, spaces[-1], mass, ceed.coefficient_context(3))
    local = [fine.coarsen(geom, s) for s in spaces[:-1]] + [fine]
    conf = [linalg.Conforming(ctx, s) for s in spaces]
    A = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE, conforming=c) for op, s, c in zip(local, spaces, conf)]
    P = [linalg.Interp(ctx, a, b, conforming=c) for a, b, c in zip(spaces[:-1], spaces[1:], conf[:-1])]
    return ctx, spaces, A, P, (geom, local, conf)


def _python_solve(mirror, coarse):
    import torch

    from palace_amd import linalg

    ctx, spaces, A, P, _ = mirror
    if coarse == "pcg":
        cs = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1e-2, max_it=8)
    elif coarse == "jacobi":
        cs = linalg.jacobi(ctx, A[0])
    else:
        cs = linalg.chebyshev(ctx, A[0], 4)
    B = linalg.gmg(ctx, A, P, cs, cheby_order=4)   # mg_smooth_order = max(2 * order, 4)
    K = linalg.cg(ctx, A[-1], B, rel_tol=1e-10, max_it=400)
    n = spaces[-1].n_true
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    b = torch.empty_like(ones)
    A[-1].mult(ones, b)
    b[torch.from_numpy(spaces[-1].ess_dofs().astype(np.int64)).cuda()] = 0.0
    x = torch.zeros_like(b)
    K.mult(b, x)
    assert K.stats()["converged"]
    return n, K.stats()["iterations"], float(x.sum())


@pytest.mark.parametrize("coarse", ["pcg", "cheb", "jacobi"])
def test_cxx_nc_solve(built, mirror, coarse):
    """KspSolver with JACOBI_PCG, CHEBYSHEV_JACOBI or JACOBI at the constrained level 0."""
    exe, blob = built
    out = subprocess.check_output([exe, blob, coarse], text=True)
    m = re.search(r"ndofs (\d+)\s+constrained (\d+) .* iterations (\d+)\s+converged (\d)\s+\|b - A x\| / \|b\| (\S+)\s+sum\(x\) (\S+)", out)
    assert m, out
    n, ncon, its, conv = (int(m.group(i)) for i in range(1, 5))
    res, sx = float(m.group(5)), float(m.group(6))
    assert conv == 1 and res < 1e-8 and ncon > 0, out
    n_py, its_py, sx_py = _python_solve(mirror, coarse)
    print(out.strip(), "| mirror:", n_py, its_py, sx_py)
    assert n == n_py and ncon == mirror[1][-1].n_local - n_py
    assert abs(its - its_py) <= 1, (out, its_py)
    assert abs(sx - sx_py) < 1e-6 * abs(sx_py)


def test_cxx_nc_amg_is_refused(built):
    """BOOMER_AMG on a constrained level 0 needs the assembled P^T A P: a clear error, not a wrong matrix."""
    exe, blob = built
    r = subprocess.run([exe, blob, "amg"], capture_output=True, text=True)
    assert r.returncode == 1 and "hanging-node constraints" in r.stderr and "JACOBI_PCG" in r.stderr, r.stderr
