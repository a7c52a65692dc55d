"""The algebraic coarse solvers on a level with hanging-node constraints, fed by the device triple product
(palace_amd/csrc/pa_rap_conform.hip): AMG on the constrained H1 space and AMS on the constrained Nedelec space of the refined
cylinder (mesh C of tests/nc_util.py) at order 1, each against the same solver built on scipy's P^T A P (and gradient) uploaded
with DeviceCsr.from_scipy -- iterations +-1 (the project's criterion), both converged, solutions to 1e-6 -- and p-multigrid
[1, 2] with AMS at an assembled level 0 against the same hierarchy with the Jacobi-PCG level-0 solve."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import vertex_coordinates  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import util  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


def _pcg(ctx, A, B, ess, rel_tol=1e-10, max_it=400):
    """A x = b with b = A 1 (essential rows zero): (iterations, converged, x)."""
    n = A.n
    b = A.mult(torch.ones(n, dtype=torch.float64, device="cuda"), _new(n))
    b[torch.from_numpy(np.asarray(ess, dtype=np.int64)).cuda()] = 0.0
    K = linalg.cg(ctx, A, B, rel_tol=rel_tol, max_it=max_it)
    x = K.mult(b, _new(n))
    st = K.stats()
    return st["iterations"], bool(st["converged"]), x.cpu().numpy()


def h1_level(ctx):
    """H1 diffusion + mass on mesh C at order 1: (space, local operator, Conforming, constrained ParOperator)."""
    s = nu.nc_space("C", "h1", 1)
    c_mass = po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([2.08])], dim=1)
    local = ceed.diffusionmass_operator(ceed.GeomFactorData(s.mesh, 2), s, c_mass.pack(), util.make_ctx("identity")[0].pack())
    conf = linalg.Conforming(ctx, s)
    return s, local, conf, linalg.ParOperator(ctx, local, s.ess_dofs(), linalg.DIAG_ONE, conforming=conf)


def nd_levels(ctx, orders=(1, 2)):
    """ND K + M on mesh C as tests/test_cxx_nc_gpu.py::mirror builds it: (spaces, local operators, Conformings, constrained
    ParOperators, transfers)."""
    spaces = [nu.nc_space("C", "nd", p) for p in orders]
    geom = ceed.GeomFactorData(spaces[0].mesh, orders[-1] + 1)
    mass = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[np.array([2.08])])
    fine = ceed.curlcurlmass_operator(geom, spaces[-1], mass, ceed.coefficient_context(3))
    local = [fine.coarsen(geom, s) for s in spaces[:-1]] + [fine]
    conf = [linalg.Conforming(ctx, s) for s in spaces]
    A = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE, conforming=c) for op, s, c in zip(local, spaces, conf)]
    P = [linalg.Interp(ctx, a, b, conforming=c) for a, b, c in zip(spaces[:-1], spaces[1:], conf[:-1])]
    return spaces, local, conf, A, P, geom


def true_gradient(ctx, nd, conf_nd):
    """(device R_nd G_local P_h1 as scipy, the scipy one, the true-vertex coordinates) of the lowest-order pair on nd's mesh."""
    h1 = nu.nc_space("C", "h1", 1)
    Gl = nu.local_gradient(h1, nd)
    G_dev = linalg.rap_conforming(ctx, ceed.DeviceCsr.from_scipy(Gl), test=conf_nd, trial=linalg.Conforming(ctx, h1), injection=True)
    G_ref = (Gl @ h1.prolongation()).tocsr()[:nd.n_true]
    xyz = vertex_coordinates(h1)[:h1.n_true]     # true dofs first: the true vertices
    return G_dev.to_scipy(), G_ref, xyz


def test_amg_on_constrained_h1_level(ctx):
    s, local, conf, A_free = h1_level(ctx)
    ess = s.ess_dofs()
    T = A_free.parallel_assemble()
    P = s.prolongation()
    T_ref = ceed.DeviceCsr.from_scipy((P.T @ local.full_assemble() @ P).tocsr(), symmetric=True)
    res = []
    for csr in (T, T_ref):
        A = linalg.AssembledParOperator(ctx, csr, ess, linalg.DIAG_ONE)
        B = linalg.amg(ctx, csr, ess, coarse_size=40)   # (below the library's default the 191 dofs would be one dense solve)
        assert len(linalg.amg_hierarchy(B)[0]) > 1
        res.append(_pcg(ctx, A, B, ess))
    (it_d, ok_d, x_d), (it_r, ok_r, x_r) = res
    print(f"AMG on P^T A P, H1 order 1, {s.n_true} true dofs ({s.n_local - s.n_true} constrained): {it_d} iterations (scipy matrix: {it_r})")
    assert ok_d and ok_r and abs(it_d - it_r) <= 1
    assert np.linalg.norm(x_d - x_r) < 1e-6 * np.linalg.norm(x_r)
    # ... and it solves the constrained problem: the residual of the three-launch operator
    b = A_free.mult(_dev(np.ones(s.n_true)), _new(s.n_true)).cpu().numpy()
    b[ess] = 0.0
    r = A_free.mult(_dev(x_d), _new(s.n_true)).cpu().numpy() - b
    assert np.linalg.norm(r) < 1e-8 * np.linalg.norm(b)


def test_ams_on_constrained_nd_level(ctx):
    spaces, local, conf, A_free, _, _ = nd_levels(ctx, (1,))
    nd, ess = spaces[0], spaces[0].ess_dofs()
    T = A_free[0].parallel_assemble()
    G_dev, G_ref, xyz = true_gradient(ctx, nd, conf[0])
    assert np.diff(G_dev.indptr).max() > 2      # not an incidence matrix: edges into hanging vertices
    P = nd.prolongation()
    T_ref = ceed.DeviceCsr.from_scipy((P.T @ local[0].full_assemble() @ P).tocsr(), symmetric=True)
    res = []
    for csr, G in ((T, G_dev), (T_ref, G_ref)):
        A = linalg.AssembledParOperator(ctx, csr, ess, linalg.DIAG_ONE)
        res.append(_pcg(ctx, A, linalg.ams(ctx, csr, ess, G, xyz), ess))
    (it_d, ok_d, x_d), (it_r, ok_r, x_r) = res
    print(f"AMS on P^T A P, ND order 1, {nd.n_true} true dofs ({nd.n_local - nd.n_true} constrained): {it_d} iterations (scipy inputs: {it_r})")
    assert ok_d and ok_r and abs(it_d - it_r) <= 1
    assert np.linalg.norm(x_d - x_r) < 1e-6 * np.linalg.norm(x_r)
    b = A_free[0].mult(_dev(np.ones(nd.n_true)), _new(nd.n_true)).cpu().numpy()
    b[ess] = 0.0
    r = A_free[0].mult(_dev(x_d), _new(nd.n_true)).cpu().numpy() - b
    assert np.linalg.norm(r) < 1e-8 * np.linalg.norm(b)


def pmg_solve(ctx, levels, coarse):
    """PCG + p-multigrid [1, 2] on mesh C; coarse 'pcg': the three-launch level 0 with its Jacobi-PCG solve (what a constrained
    level 0 had before the assembled product), 'ams': the assembled level 0 with the auxiliary-space solver.  (true dofs,
    iterations, converged, sum(x))."""
    spaces, local, conf, A, P, _ = levels
    ess0 = spaces[0].ess_dofs()
    if coarse == "pcg":
        A0 = A[0]
        cs = linalg.cg(ctx, A0, linalg.jacobi(ctx, A0), rel_tol=1e-2, max_it=8)
    else:
        T0 = A[0].parallel_assemble()
        A0 = linalg.AssembledParOperator(ctx, T0, ess0, linalg.DIAG_ONE)
        G, _, xyz = true_gradient(ctx, spaces[0], conf[0])
        cs = linalg.ams(ctx, T0, ess0, G, xyz)
    B = linalg.gmg(ctx, [A0, A[1]], P, cs, cheby_order=4)
    it, ok, x = _pcg(ctx, A[-1], B, spaces[-1].ess_dofs())
    return spaces[-1].n_true, it, ok, float(x.sum())


def test_pmg_with_ams_at_level_0(ctx):
    levels = nd_levels(ctx)
    n, it_pcg, ok_pcg, sx_pcg = pmg_solve(ctx, levels, "pcg")
    n2, it_ams, ok_ams, sx_ams = pmg_solve(ctx, levels, "ams")
    print(f"p-multigrid [1, 2], {n} true dofs: AMS at the assembled level 0 {it_ams} iterations, Jacobi-PCG level 0 {it_pcg}")
    assert ok_pcg and ok_ams       # relative tolerance 1e-10
    assert it_ams <= it_pcg
    assert abs(sx_ams - sx_pcg) < 1e-6 * abs(sx_pcg)
