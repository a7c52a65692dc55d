"""ParOperator, transfers and solvers on spaces with hanging-node constraints (device conforming prolongation,
palace_amd/csrc/pa_conform.hip) against the oracle's classes with a scipy P (tests/nc_util.py), and one estimate / mark /
refine / solve step on the cylinder."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem import nchex, rthex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import util  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


_geoms = {}


def _geom(mesh, q1d):
    key = (id(mesh), q1d)
    if key not in _geoms:
        _geoms[key] = (mesh, ceed.GeomFactorData(mesh, q1d))
    return _geoms[key][1]


def _nd_pair(ctx, name, p, q1d, policy=linalg.DIAG_ONE):
    """(space, device ParOperator of K + M with the constraint, its oracle, keep-alive)."""
    s = nu.nc_space(name, "nd", p)
    cm, bm = util.make_ctx("scalar", 2)
    cc, bc = util.make_ctx("identity")
    local = ceed.curlcurlmass_operator(_geom(s.mesh, q1d), s, bm, bc)
    conf = linalg.Conforming(ctx, s)
    A = linalg.ParOperator(ctx, local, s.ess_dofs(), policy, conforming=conf)
    oA = nu.ConstrainedParOperatorOracle([nu.CLocal(s, np.concatenate([bm, bc]), q1d, cm, cc)], s.prolongation(),
                                         s.ess_dofs(), policy)
    return s, A, oA, (local, conf)


def _check_operator(s, A, oA, seed):
    rng = np.random.default_rng(seed)
    n = s.n_true
    assert A.n == n
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    ref = oA.mult(x)
    err = {}
    err["mult"] = _rel(A.mult(_dev(x), _new(n)).cpu().numpy(), ref)
    err["mult_transpose"] = _rel(A.mult_transpose(_dev(x), _new(n)).cpu().numpy(), ref)
    err["add_mult"] = _rel(A.add_mult(_dev(x), _dev(y0.copy()), -0.5).cpu().numpy(), oA.add_mult(x, y0, -0.5))
    err["eliminate_rhs"] = _rel(A.eliminate_rhs(_dev(x), _dev(y0.copy())).cpu().numpy(), oA.eliminate_rhs(x, y0))
    err["diagonal"] = _rel(A.assemble_diagonal(_new(n)).cpu().numpy(), oA.diagonal())
    xy = _dev(x.copy())
    err["in_place"] = _rel(A.mult(xy, xy).cpu().numpy(), ref)
    print(" ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert max(err.values()) < 1e-12, err
    assert not A.fuses_essential() and not A.prepare_cheby_step()


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_par_operator_block(ctx, p):
    """Mesh A, ND K + M: Mult, MultTranspose, AddMult, EliminateRHS, AssembleDiagonal against the oracle with a scipy P."""
    s, A, oA, keep = _nd_pair(ctx, "A", p, p + 1)
    _check_operator(s, A, oA, p)
    y = A.mult(_dev(np.ones(s.n_true)), _new(s.n_true)).cpu().numpy()
    assert np.array_equal(y[s.ess_dofs()], np.ones(s.ess_dofs().size))   # DIAG_ONE rows: a copy


def test_par_operator_diag_zero(ctx):
    s, A, oA, keep = _nd_pair(ctx, "A", 2, 3, linalg.DIAG_ZERO)
    _check_operator(s, A, oA, 7)


def test_par_operator_h1(ctx):
    """Mesh A, H1 diffusion + mass, order 2."""
    s = nu.nc_space("A", "h1", 2)
    c_mass = po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([2.08])], dim=1)
    c_diff = util.make_ctx("identity")[0]
    local = ceed.diffusionmass_operator(_geom(s.mesh, 3), s, c_mass.pack(), c_diff.pack())
    conf = linalg.Conforming(ctx, s)
    A = linalg.ParOperator(ctx, local, s.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
    oA = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hcurlmass", c_mass, c_diff, 3)], s.prolongation(), s.ess_dofs())
    _check_operator(s, A, oA, 11)


def test_par_operator_cylinder_order_5(ctx):
    """Mesh C, order 5, six points per direction."""
    s, A, oA, keep = _nd_pair(ctx, "C", 5, 6)
    _check_operator(s, A, oA, 5)


def test_par_sum_operator(ctx):
    s = nu.nc_space("A", "nd", 2)
    cm, bm = util.make_ctx("scalar", 2)
    cc, bc = util.make_ctx("identity")
    geom = _geom(s.mesh, 3)
    K, M = ceed.curlcurl_operator(geom, s, bc), ceed.ndmass_operator(geom, s, bm)
    conf = linalg.Conforming(ctx, s)
    A = linalg.ParSumOperator(ctx, [K, M], [1.0, -0.3], s.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
    oK = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hdiv", cc, None, 3)], s.prolongation(), [])
    oM = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hcurl", cm, None, 3)], s.prolongation(), [])
    x = np.random.default_rng(2).uniform(-1, 1, s.n_true)
    tx = x.copy()
    tx[s.ess_dofs()] = 0.0
    ref = oK.mult(tx) - 0.3 * oM.mult(tx)
    ref[s.ess_dofs()] = x[s.ess_dofs()]
    assert _rel(A.mult(_dev(x), _new(s.n_true)).cpu().numpy(), ref) < 1e-12


def test_complex_par_operator(ctx):
    """(K + M) + i M with the constraint: the two real ParOperators carry P."""
    s = nu.nc_space("A", "nd", 2)
    cm, bm = util.make_ctx("scalar", 2)
    cc, bc = util.make_ctx("identity")
    geom = _geom(s.mesh, 3)
    Ar, Ai = ceed.curlcurlmass_operator(geom, s, bm, bc), ceed.ndmass_operator(geom, s, bm)
    conf = linalg.Conforming(ctx, s)
    ess = s.ess_dofs()
    A = linalg.ComplexParOperator(ctx, Ar, Ai, ess, linalg.DIAG_ONE, conforming=conf)
    P = s.prolongation()
    oR = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hdivmass", cm, cc, 3)], P, ess, po.DIAG_ONE)
    oI = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hcurl", cm, None, 3)], P, ess, po.DIAG_ZERO)
    rng = np.random.default_rng(4)
    xr, xi = rng.uniform(-1, 1, s.n_true), rng.uniform(-1, 1, s.n_true)
    yr, yi = A.mult(_dev(xr), _dev(xi), _new(s.n_true), _new(s.n_true))
    assert _rel(yr.cpu().numpy(), oR.mult(xr) - oI.mult(xi)) < 1e-12
    assert _rel(yi.cpu().numpy(), oI.mult(xr) + oR.mult(xi)) < 1e-12


def test_halo_and_constraint_together_are_refused(ctx):
    s = nu.nc_space("A", "nd", 2)
    with pytest.raises(ValueError, match="together"):
        linalg.ParOperator(ctx, None, [], conforming=object(), halo=object())
    # the C entry point checks the sizes of the constraint against the operator
    other = linalg.Conforming(ctx, nu.nc_space("A", "h1", 2))
    local = ceed.ndmass_operator(_geom(s.mesh, 3), s, util.make_ctx("identity")[1])
    with pytest.raises(Exception, match="does not match"):
        linalg.ParOperator(ctx, local, [], conforming=other)


# ---- solvers -------------------------------------------------------------------------------------------

class Hierarchy:
    """K + M on mesh C at orders `levels` with the constraint on every level: device and oracle side by side."""

    def __init__(self, ctx, levels):
        self.ctx, self.levels = ctx, levels
        q1d = levels[-1] + 1
        self.spaces = [nu.nc_space("C", "nd", p) for p in levels]
        cm, bm = util.make_ctx("scalar", 2)
        cc, bc = util.make_ctx("identity")
        geom = _geom(self.spaces[0].mesh, q1d)
        fine = ceed.curlcurlmass_operator(geom, self.spaces[-1], bm, bc)
        self.local = [fine.coarsen(geom, s) for s in self.spaces[:-1]] + [fine]
        self.conf = [linalg.Conforming(ctx, s) for s in self.spaces]
        self.A = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE, conforming=c)
                  for op, s, c in zip(self.local, self.spaces, self.conf)]
        blob = np.concatenate([bm, bc])
        self.oA = [nu.ConstrainedParOperatorOracle([nu.CLocal(s, blob, q1d, cm, cc)], s.prolongation(), s.ess_dofs())
                   for s in self.spaces]
        self.P = [linalg.Interp(ctx, a, b, conforming=c) for a, b, c in zip(self.spaces[:-1], self.spaces[1:], self.conf[:-1])]
        self.oP = []
        for a, b in zip(self.spaces[:-1], self.spaces[1:]):
            I = po.InterpOracle(a.elem_dof_lex, a.elem_sign_lex, b.elem_dof_lex, b.elem_sign_lex, a.ndofs, b.ndofs,
                                po.nd_hex_interp_lex(a.p, b.p))
            Pc = a.prolongation()
            # R_f I P_c and P_c^T I^T R_f^T (zero-filled tail)
            self.oP.append((lambda x, I=I, Pc=Pc, b=b: I.mult(Pc @ x)[:b.n_true],
                            lambda y, I=I, Pc=Pc, b=b: Pc.T @ I.mult_transpose(np.concatenate([y, np.zeros(b.n_local - b.n_true)]))))


@pytest.fixture(scope="module")
def hier(ctx):
    return Hierarchy(ctx, [1, 2, 3])


def test_transfers(hier):
    rng = np.random.default_rng(6)
    for l, (P, (om, omt)) in enumerate(zip(hier.P, hier.oP)):
        nc, nf = hier.spaces[l].n_true, hier.spaces[l + 1].n_true
        xc, xf = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf)
        yf = P.mult(_dev(xc), _new(nf)).cpu().numpy()
        yc = P.mult_transpose(_dev(xf), _new(nc)).cpu().numpy()
        assert _rel(yf, om(xc)) < 1e-13 and _rel(yc, omt(xf)) < 1e-13
        assert abs(xf @ yf - xc @ yc) < 1e-12 * abs(xf @ yf)


def test_gradient_with_constraints(ctx):
    """R_nd G P_h1 on true-dof vectors, and its transpose."""
    nd, h1 = nu.nc_space("C", "nd", 2), nu.nc_space("C", "h1", 2)
    G = linalg.Gradient(ctx, h1, nd, conforming=linalg.Conforming(ctx, h1))
    Gl = nu.local_gradient(h1, nd)
    rng = np.random.default_rng(9)
    xh, xn = rng.uniform(-1, 1, h1.n_true), rng.uniform(-1, 1, nd.n_true)
    ref = (Gl @ (h1.prolongation() @ xh))[:nd.n_true]
    assert _rel(G.mult(_dev(xh), _new(nd.n_true)).cpu().numpy(), ref) < 1e-13
    reft = h1.prolongation().T @ (Gl.T @ np.concatenate([xn, np.zeros(nd.n_local - nd.n_true)]))
    assert _rel(G.mult_transpose(_dev(xn), _new(h1.n_true)).cpu().numpy(), reft) < 1e-13


def test_pcg_jacobi_matches_oracle(hier):
    """Mesh C, order 2: iteration count +-1 and solution against oracle.pcg on the assembled P^T A P (held in CSR: the same
    matrix as the dense one, rows and columns of the essential dofs eliminated), with the gate of test_solvers_gpu.py."""
    l = 1
    s, oA = hier.spaces[l], hier.oA[l]
    n, ess = s.n_true, s.ess_dofs()
    P = s.prolongation()
    Al = oA.ops[0].np_op.assemble_sparse().tocsr()
    keep = np.ones(n)
    keep[ess] = 0.0
    import scipy.sparse as sp
    D = sp.diags(keep)
    PAP = (D @ (P.T @ Al @ P) @ D + sp.diags(1.0 - keep)).tocsr()
    x0 = np.random.default_rng(12).uniform(-1, 1, n)
    assert _rel(PAP @ x0, oA.mult(x0)) < 1e-12
    b = oA.mult(np.ones(n))
    b[ess] = 0.0
    K = linalg.cg(hier.ctx, hier.A[l], linalg.jacobi(hier.ctx, hier.A[l]), rel_tol=1e-8, max_it=500)
    x = K.mult(_dev(b), _new(n)).cpu().numpy()
    dinv = 1.0 / oA.diagonal()
    xo, it, hist = po.pcg(lambda v: PAP @ v, b, lambda r: dinv * r, rel_tol=1e-8, max_it=500)
    st = K.stats()
    print(st, it)
    assert st["converged"] and abs(st["iterations"] - it) <= 1
    assert _rel(x, xo) < 1e-6
    assert np.linalg.norm(oA.mult(x) - b) < 1e-6 * np.linalg.norm(b)


def test_gmg_vcycle_and_pcg(hier):
    """p-multigrid (1, 2, 3), Chebyshev smoothing, Jacobi-PCG at level 0, on the constrained hierarchy: the V-cycle against
    GMGOracle on the constrained oracle operators, then PCG iteration counts and solution (tolerances of the conforming case)."""
    n = hier.spaces[-1].n_true
    coarse = linalg.cg(hier.ctx, hier.A[0], linalg.jacobi(hier.ctx, hier.A[0]), rel_tol=1e-3, max_it=200)
    B = linalg.gmg(hier.ctx, hier.A, hier.P, coarse, cheby_order=6)
    for l in (1, 2):
        assert not B.fused_step(l)   # the constrained operator has no fused smoother step: the plain path, no throw
    lam = [linalg.chebyshev(hier.ctx, hier.A[l], order=6).lambda_max() for l in (1, 2)]
    sm = [None] + [po.ChebyshevOracle(hier.oA[l], 6, lambda_max=lam[l - 1]) for l in (1, 2)]
    d0 = 1.0 / hier.oA[0].diagonal()
    ocoarse = lambda r: po.pcg(hier.oA[0].mult, r, lambda v: d0 * v, rel_tol=1e-3, max_it=200)[0]  # noqa: E731
    oB = po.GMGOracle(hier.oA, hier.oP, sm, ocoarse, [s.ess_dofs() for s in hier.spaces])
    ess = hier.spaces[-1].ess_dofs()
    r = np.random.default_rng(8).uniform(-1, 1, n)
    r[ess] = 0.0
    z = B.mult(_dev(r), _new(n)).cpu().numpy()
    print(f"vcycle {_rel(z, oB.mult(r)):.2e}")
    assert _rel(z, oB.mult(r)) < 1e-8
    b = hier.oA[-1].mult(np.ones(n))
    b[ess] = 0.0
    K = linalg.cg(hier.ctx, hier.A[-1], B, rel_tol=1e-8, max_it=200)
    x = K.mult(_dev(b), _new(n)).cpu().numpy()
    xo, it, hist = po.pcg(hier.oA[-1].mult, b, oB.mult, rel_tol=1e-8, max_it=200)
    st = K.stats()
    print(st, it)
    assert st["converged"] and abs(st["iterations"] - it) <= 1, (st, it)
    assert _rel(x, xo) < 1e-6


# ---- estimate, mark, refine, solve ---------------------------------------------------------------------

def _smooth_field(x):
    return np.stack([np.sin(0.7 * x[..., 1]) * np.cos(0.4 * x[..., 2]), np.cos(0.5 * x[..., 0] + 0.3) * np.sin(0.6 * x[..., 2] + 0.2),
                     np.sin(0.4 * x[..., 0]) * np.cos(0.8 * x[..., 1])], axis=-1)


def _solve(ctx, space, conf):
    """(K + M) u = M f with PEC walls, f the interpolant of a smooth field: (true-dof solution, solver statistics, keep-alive)."""
    ident = util.make_ctx("identity")[1]
    geom = _geom(space.mesh, 3)
    A_loc, M_loc = ceed.curlcurlmass_operator(geom, space, ident, ident), ceed.ndmass_operator(geom, space, ident)
    n_local = space.ndofs
    f = util.nd_interpolate(space, _smooth_field)
    lb = M_loc.mult(_dev(f), _new(n_local))
    n = n_local if conf is None else conf.n_true
    if conf is None:
        b = lb.clone()
        A = linalg.ParOperator(ctx, A_loc, space.ess_dofs(), linalg.DIAG_ONE)
    else:
        b = conf.restrict(lb, _new(n))
        A = linalg.ParOperator(ctx, A_loc, space.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
    b[torch.from_numpy(space.ess_dofs().astype(np.int64)).cuda()] = 0.0
    K = linalg.cg(ctx, A, linalg.jacobi(ctx, A), rel_tol=1e-10, max_it=2000)
    x = K.mult(b, _new(n))
    return x, K.stats(), (A, A_loc, M_loc, K)


def test_estimate_mark_refine_solve(ctx):
    """One step of SolveEstimateMarkRefine (drivers/basesolver.cpp) on the cylinder at order 2: solve, CurlFluxErrorEstimator
    through the Python mirror, Doerfler marking at 0.7, local refinement, solve on the constrained space.  The second solve
    converges, and its solution, evaluated at the coarse mesh's dof nodes through P and the children's bases
    (nchex.coarse_node_values, the left inverse of the child-matrix transfer), differs from the first -- relative l2 norm of the
    dof vectors -- by less than the first solve's estimated relative error (a sanity bound from the estimator, no rate claim).
    Measured: 22 of 80 elements marked (the closure adds none), estimated relative error 6.29e-2, moved at the coarse dof nodes
    7.7e-3.  For the record the same difference in the curl seminorm on the refined mesh, the quantity the estimator measures,
    is printed too (6.03e-2)."""
    from tests.test_mixed_hex_gpu import device_estimate

    p = 2
    m0 = nu.start_mesh("C")
    s0 = NDHexSpace(m0, p)
    x1, st1, keep1 = _solve(ctx, s0, None)
    assert st1["converged"]
    # B = curl A in the Raviart-Thomas space, then the flux error estimate eta_e^2 with mu = 1
    rt = rthex.RTHexSpace(m0, p)
    Bf = linalg.Curl(ctx, s0, rt).mult(x1, _new(rt.ndofs))
    est, _, _ = device_estimate(m0, p, "curl", Bf.cpu().numpy(), [np.eye(3)])
    assert est.min() >= 0.0 and est.max() > 0.0
    Mrt = ceed.rtmass_operator(_geom(m0, 3), rt, util.make_ctx("identity")[1])
    norm2 = float(Bf @ Mrt.mult(Bf, _new(rt.ndofs)))
    est_rel = np.sqrt(est.sum() / norm2)
    marked = nchex.dorfler_mark(np.sqrt(est), 0.7)
    assert 0 < marked.size < m0.ne
    m1 = nchex.refine_local(m0, marked)
    assert m1.master_faces.size > 0 and set(marked.tolist()) <= set(m1.marked.tolist())
    s1 = nchex.NCSpace(NDHexSpace(m1, p))
    conf = linalg.Conforming(ctx, s1)
    x2, st2, keep2 = _solve(ctx, s1, conf)
    print(st1, st2)
    assert st2["converged"]
    # both solutions as local vectors of the refined mesh
    u2 = s1.prolongation() @ x2.cpu().numpy()
    u1 = nchex.refinement_transfer(s0, s1) @ x1.cpu().numpy()
    Kf = ceed.curlcurl_operator(_geom(m1, 3), s1, util.make_ctx("identity")[1])
    semi = lambda u: float(np.sqrt(u @ Kf.mult(_dev(u), _new(s1.ndofs)).cpu().numpy()))  # noqa: E731
    # the second solution at the coarse mesh's dof nodes (through P, then the children's bases at those nodes), against the first
    x1h = x1.cpu().numpy()
    at_nodes = nchex.coarse_node_values(s0, s1, u2)
    moved = np.linalg.norm(at_nodes - x1h) / np.linalg.norm(x1h)
    # (the transfer and the node values are consistent: the first solution goes to the refined mesh and back unchanged)
    assert np.abs(nchex.coarse_node_values(s0, s1, u1) - x1h).max() < 1e-12 * np.abs(x1h).max()
    moved_semi = semi(u2 - u1) / semi(u1)
    print(f"marked {marked.size} of {m0.ne} (closed: {m1.marked.size}), estimated relative error {est_rel:.3e}, moved at the coarse "
          f"dof nodes {moved:.3e}, in the curl seminorm on the refined mesh {moved_semi:.3e}")
    print(f"curl norm of the first solution on the two meshes: {abs(semi(u1) ** 2 - norm2) / norm2:.2e}")
    # the transfer keeps the function: same curl norm on the refined mesh, up to the quadrature error of the curved elements
    # that were split (measured 1.2e-4)
    assert abs(semi(u1) ** 2 - norm2) < 1e-3 * norm2
    assert 0.0 < moved < est_rel
