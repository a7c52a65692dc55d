"""The C++ host layer at order 5: examples/cxx_host/solve.cpp on dump_problem.py's 15-element cavity with the levels
[1, 2, 3, 5] of the reference's logarithmic coarsening -- FiniteElementSpaceHierarchy, BilinearForm::Assemble, KspSolver on
the six-point element kernels -- against the same solve through the ctypes mirror (criteria of tests/test_cxx_host_gpu.py:
iterations +- 1, checksum 1e-6).  Plain Chebyshev smoothing with a Jacobi-PCG coarse solve, and Hiptmair smoothing with AMS
on the assembled (1, 6) matrix: the second runs the H1 kernels at (1, 6) ... (5, 6) and the order-5 discrete gradient."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER, N, NZ = 5, 1, 3


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("cxx_hex_q6")
    exe, blob = str(d / "solve"), str(d / "problem.bin")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "examples", "cxx_host", "dump_problem.py"), blob, str(ORDER), str(N),
                           str(NZ)])
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cxx_host", "solve.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", exe])
    return exe, blob


def _python_solve(aux, coarse):
    import torch

    from palace_amd import ceed, linalg
    from palace_amd.fem.fespace import H1HexSpace, NDHexSpace
    from palace_amd.fem.mesh import ogrid_cylinder
    from palace_amd.fem.partition import levels_for

    ctx = linalg.Context()
    mesh = ogrid_cylinder(N, NZ)
    orders = levels_for(ORDER)
    assert orders == [1, 2, 3, 5] and mesh.ne == 15
    nds = [NDHexSpace(mesh, p) for p in orders]
    geom = ceed.GeomFactorData(mesh, ORDER + 1)
    mass = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[np.array([2.08])])
    fine = ceed.curlcurlmass_operator(geom, nds[-1], mass, ceed.coefficient_context(3))
    local = [fine.coarsen(geom, s) for s in nds[:-1]] + [fine]
    A = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE) for op, s in zip(local, nds)]
    A[0] = linalg.AssembledParOperator(ctx, local[0].full_assemble_device(), nds[0].ess_dofs(), linalg.DIAG_ONE)
    P = [linalg.Interp(ctx, a, b) for a, b in zip(nds[:-1], nds[1:])]
    kw, keep = {}, []
    if aux:
        h1s = [H1HexSpace(mesh, p) for p in orders]
        fine_h1 = ceed.diffusion_operator(geom, h1s[-1], mass)
        loc_h1 = [fine_h1.coarsen(geom, s) for s in h1s[:-1]] + [fine_h1]
        A_h1 = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE) for op, s in zip(loc_h1, h1s)]
        G = [linalg.Gradient(ctx, h, n) for h, n in zip(h1s, nds)]
        kw, keep = dict(A_aux=A_h1, G=G), [h1s, loc_h1]
    if coarse == "ams":
        from palace_amd.fem.fespace import lowest_order_gradient, vertex_coordinates

        h1_0 = H1HexSpace(mesh, 1)
        cs = linalg.ams(ctx, A[0].local, nds[0].ess_dofs(), lowest_order_gradient(h1_0, nds[0]), vertex_coordinates(h1_0))
    else:
        cs = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1e-2, max_it=8)
    B = linalg.gmg(ctx, A, P, cs, cheby_order=max(2 * ORDER, 4), **kw)  # LinearSolverData::SetDefaults: MGSmoothOrder
    K = linalg.cg(ctx, A[-1], B, rel_tol=1e-10, max_it=400)
    n = nds[-1].ndofs
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    b = torch.empty_like(ones)
    A[-1].mult(ones, b)
    b[torch.from_numpy(nds[-1].ess_dofs().astype(np.int64)).cuda()] = 0.0
    x = torch.zeros_like(b)
    K.mult(b, x)
    return n, K.stats()["iterations"], float(x.sum())


@pytest.mark.parametrize("aux,coarse", [(0, "pcg"), (1, "ams")])
def test_cxx_host_solve_at_order_five(built, aux, coarse):
    exe, blob = built
    out = subprocess.check_output([exe, blob, str(aux), "cg", coarse], text=True)
    m = re.search(r"order (\d+)\s+levels (\d+)\s+ndofs (\d+) .* iterations (\d+)\s+converged (\d)\s+NumTotalMult (\d+)\s+"
                  r"NumTotalMultIterations (\d+)\s+\|b - A x\| / \|b\| (\S+)\s+sum\(x\) (\S+)", out)
    assert m, out
    order, nlev, n, its, conv = (int(m.group(i)) for i in range(1, 6))
    res, sx = float(m.group(8)), float(m.group(9))
    assert order == 5 and nlev == 4 and conv == 1 and res < 1e-8, out
    n_py, its_py, sx_py = _python_solve(aux, coarse)
    print(f"C++: {its} iterations, sum(x) {sx!r}; mirror: {its_py}, {sx_py!r}")
    assert n == n_py and abs(its - its_py) <= 1, (out, its_py)
    assert abs(sx - sx_py) < 1e-6 * abs(sx_py)
