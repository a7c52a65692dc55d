"""The flux error estimates on hexahedral meshes with hanging nodes, through the Python mirror: the smooth flux is the solution of
P_s^T M P_s G = P_s^T Flux P_r F (PCG + Jacobi on |P|^T diag), the element integrator takes P_r F and P_s G.  Real and complex
fields, grad-flux (F in H(curl), G in H(div)) and curl-flux (the other way round), element by element against the same procedure
through the oracle's local operators, the scipy prolongations and a direct solve of P^T M P.  Tolerance and projector settings:
those of tests/test_mixed_hex_gpu.py::test_flux_error_estimate (the same quantity on a conforming mesh)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import rt_nc_util as rn  # noqa: E402
from tests import rthex_util as ru  # noqa: E402
from tests import test_mixed_hex_gpu as mh  # noqa: E402
from tests import util  # noqa: E402

TOL = 1e-9          # test_flux_error_estimate: smooth flux and estimates
REL_TOL, MAX_IT = 1e-13, 1000
CASES = [("C", 2), ("A", 1), ("A", 3)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


class NCEstimator:
    """The pieces of one estimator on the constrained spaces (nd, rt) of one mesh and order, on the device."""

    def __init__(self, ctx, nd, rt, direction, mats=None):
        self.ctx, self.direction = ctx, direction
        self.rhs_sp, self.smooth = (nd, rt) if direction == "grad" else (rt, nd)
        c_mat, c_sq, c_isq = mh.estimator_materials(mats)
        p = nd.p
        self.geom = ceed.GeomFactorData(nd.mesh, p + 1)
        self.flux = ceed.mixedmass_operator(self.geom, self.rhs_sp, self.smooth, c_mat.pack())
        self.mass = (ceed.rtmass_operator if direction == "grad" else ceed.ndmass_operator)(self.geom, self.smooth, po.CoeffCtx().pack())
        self.c_rhs, self.c_sm = linalg.Conforming(ctx, self.rhs_sp), linalg.Conforming(ctx, self.smooth)
        self.M = linalg.ParOperator(ctx, self.mass, np.zeros(0, np.int32), linalg.DIAG_ONE, conforming=self.c_sm)
        self.cg = linalg.cg(ctx, self.M, linalg.jacobi(ctx, self.M), rel_tol=REL_TOL, max_it=MAX_IT)
        qf = ceed.QF_HCURLHDIV_ERROR_33 if direction == "grad" else ceed.QF_HDIVHCURL_ERROR_33
        self.integ = ceed.HexElementErrorIntegrator(self.geom, self.rhs_sp, self.smooth, qf, np.concatenate([c_sq.pack(), c_isq.pack()]))

    def project(self, F):
        """(P_r F, G, iterations) for a true-dof field F on the device."""
        lF = self.c_rhs.prolongate(F, _new(self.rhs_sp.n_local))
        ly = self.flux.mult(lF, _new(self.smooth.n_local))
        rhs = self.c_sm.restrict(ly, _new(self.smooth.n_true))
        G = self.cg.mult(rhs, _new(self.smooth.n_true))
        assert self.cg.stats()["converged"]
        return lF, G, self.cg.stats()["iterations"]

    def estimate_device(self, F):
        """The same for a device tensor, nothing copied back: (estimates, smooth flux, iterations)."""
        lF, G, its = self.project(F)
        lG = self.c_sm.prolongate(G, _new(self.smooth.n_local))
        return self.integ.apply_add(lF, lG, _new(self.integ.ne)), G, its

    def estimate(self, field):
        """(estimates [NE], smooth flux on the true dofs, PCG iterations) of a real true-dof field."""
        est, G, its = self.estimate_device(_dev(field))
        return est.cpu().numpy(), G.cpu().numpy(), its

    def estimate_complex(self, field_r, field_i):
        """Both parts together: prolongate2, mult2, restrict2, ComplexParCg on the constrained mass, apply_add2."""
        Fr, Fi = _dev(field_r), _dev(field_i)
        nl_r, nl_s, nt_s = self.rhs_sp.n_local, self.smooth.n_local, self.smooth.n_true
        lFr, lFi = self.c_rhs.prolongate2(Fr, Fi, _new(nl_r), _new(nl_r))
        lyr, lyi = self.flux.mult2(lFr, lFi, _new(nl_s), _new(nl_s))
        br, bi = self.c_sm.restrict2(lyr, lyi, _new(nt_s), _new(nt_s))
        Mc = linalg.ComplexParOperator(self.ctx, self.mass, None, conforming=self.c_sm)
        cg = linalg.ComplexParCg(self.ctx, Mc, linalg.jacobi(self.ctx, self.M), rel_tol=REL_TOL, max_it=MAX_IT)
        Gr, Gi = _new(nt_s), _new(nt_s)
        cg.mult(br, bi, Gr, Gi)
        assert cg.stats()["converged"]
        lGr, lGi = self.c_sm.prolongate2(Gr, Gi, _new(nl_s), _new(nl_s))
        est = self.integ.apply_add2(lFr, lGr, lFi, lGi, _new(self.integ.ne))
        return est.cpu().numpy(), (Gr.cpu().numpy(), Gi.cpu().numpy()), cg.stats()["iterations"]


_oracles = {}


def oracle_pieces(nd, rt, direction, mats=None):
    """(dense P_s^T M P_s, x -> P_s^T Flux P_r x, (F, G) -> element errors) through the oracle's local operators and scipy Ps."""
    key = (id(nd), id(rt), direction)
    if key not in _oracles:
        p, q1d = nd.p, nd.p + 1
        og = util.oracle_geom(nd.mesh, q1d)
        off, ori = nd.native_restriction()
        nint, ncurl = util.dense_tables(nd, q1d)
        nint, ncurl = np.asarray(nint).reshape(3, -1, nd.P), np.asarray(ncurl).reshape(3, -1, nd.P)
        rint, _ = ru.tables(p, q1d)
        ndo = po.CeedOperatorOracle(nd.ndofs, off, ori, nint, ncurl, og, po.QF_HCURL, None)
        rto = po.CeedOperatorOracle(rt.ndofs, rt.elem_dof_lex, rt.elem_sign_lex < 0, rint, rint, og, po.QF_HDIV, None)
        (s1, o1), (s2, o2) = ((nd, ndo), (rt, rto)) if direction == "grad" else ((rt, rto), (nd, ndo))
        c_mat, c_sq, c_isq = mh.estimator_materials(mats)
        Mo = po.CeedOperatorOracle(o2.lsize, o2.off, o2.sgn < 0, o2.interp, o2.interp, og,
                                   po.QF_HDIV if direction == "grad" else po.QF_HCURL, po.CoeffCtx())
        P1, P2 = s1.prolongation(), s2.prolongation()
        PMP = (P2.T @ Mo.assemble_sparse().tocsr() @ P2).toarray()
        qfo, qfe = ((po.QF_HCURLHDIV, po.QF_HCURLHDIV_ERROR) if direction == "grad" else (po.QF_HDIVHCURL, po.QF_HDIVHCURL_ERROR))
        flux = po.MixedSpaceOracle(o1, o2, og, qfo, c_mat)
        err = po.MixedSpaceOracle(o1, o2, og, qfe, c_sq, c_isq)
        _oracles[key] = (nd, rt, PMP, P1, P2, flux, err, s2, o1)
    return _oracles[key][2:]


def oracle_estimate(nd, rt, direction, field, mats=None):
    PMP, P1, P2, flux, err, s2, o1 = oracle_pieces(nd, rt, direction, mats)
    lF = P1 @ field
    G = np.linalg.solve(PMP, P2.T @ flux.apply_add(lF, np.zeros(s2.n_local)))
    return err.error_add(lF, P2 @ G, np.zeros(o1.NE)), G


def _field(space, seed):
    return np.random.default_rng(seed).uniform(-1, 1, space.n_true)


@pytest.mark.parametrize("direction", ["grad", "curl"])
@pytest.mark.parametrize("name,p", CASES)
def test_flux_error_estimate(ctx, name, p, direction):
    nd, rt = nu.nc_space(name, "nd", p), rn.rt_space(name, p)
    E = _field(nd if direction == "grad" else rt, 70 + p)
    est, G, its = NCEstimator(ctx, nd, rt, direction).estimate(E)
    est_o, G_o = oracle_estimate(nd, rt, direction, E)
    eG, ee = np.linalg.norm(G - G_o) / np.linalg.norm(G_o), np.abs(est - est_o).max() / est_o.max()
    print(f"{name} p={p} {direction}: smooth flux {eG:.2e} estimates {ee:.2e} iterations {its}")
    assert eG < TOL and ee < TOL
    assert est_o.min() > 0


@pytest.mark.parametrize("direction", ["grad", "curl"])
@pytest.mark.parametrize("name,p", CASES)
def test_complex_flux_error_estimate(ctx, name, p, direction):
    """Both parts through prolongate2 / mult2 / restrict2 / apply_add2: the oracle on each part, and the sum of two real runs."""
    nd, rt = nu.nc_space(name, "nd", p), rn.rt_space(name, p)
    sp = nd if direction == "grad" else rt
    Er, Ei = _field(sp, 70 + p), _field(sp, 170 + p)
    K = NCEstimator(ctx, nd, rt, direction)
    est, (Gr, Gi), its = K.estimate_complex(Er, Ei)
    (er, Gr_r, _), (ei, Gi_r, _) = K.estimate(Er), K.estimate(Ei)
    two = np.abs(est - (er + ei)).max() / (er + ei).max()
    (eor, Gor), (eoi, Goi) = oracle_estimate(nd, rt, direction, Er), oracle_estimate(nd, rt, direction, Ei)
    ee = np.abs(est - (eor + eoi)).max() / (eor + eoi).max()
    eG = max(np.linalg.norm(Gr - Gor) / np.linalg.norm(Gor), np.linalg.norm(Gi - Goi) / np.linalg.norm(Goi))
    print(f"{name} p={p} {direction}: against two real runs {two:.2e}, against the oracle: estimates {ee:.2e} smooth flux {eG:.2e}")
    assert two < TOL and ee < TOL and eG < TOL


def test_halo_and_constraint_together_are_refused(ctx):
    rt = rn.rt_space("A", 1)
    local = ceed.rtmass_operator(ceed.GeomFactorData(rt.mesh, 2), rt, po.CoeffCtx().pack())
    with pytest.raises(ValueError, match="together"):
        linalg.ParOperator(ctx, local, [], conforming=linalg.Conforming(ctx, rt), halo=object())
    with pytest.raises(ValueError, match="together"):
        linalg.ComplexParOperator(ctx, local, None, conforming=linalg.Conforming(ctx, rt), halo=object())


# ---- solve, estimate, mark, refine: two steps ------------------------------------------------------------------------------

def _one_irregular(mesh):
    """Across every master face and edge the refinement level differs by exactly one (the topology itself refuses a hanging
    entity without its slaves, and NCSpace a chain of constraints)."""
    nc = mesh._nc()
    for f in np.nonzero(nc["face_master"] >= 0)[0]:
        M, _ = nc["mfaces"][int(nc["face_master"][f])]
        if mesh.level[nc["face_elem"][f][0]] - mesh.level[M] != 1:
            return False
    for e in np.nonzero(nc["edge_master"] >= 0)[0]:
        M, _ = nc["medges"][int(nc["edge_master"][e])]
        if mesh.level[nc["edge_elem"][e][0]] - mesh.level[M] != 1:
            return False
    return True


def test_two_step_estimate_mark_refine_solve(ctx):
    """Two steps of SolveEstimateMarkRefine (drivers/basesolver.cpp) on the 80-element cylinder at order 2, continuing
    tests/test_nc_solve_gpu.py::test_estimate_mark_refine_solve: solve (K + M) u = M f, B = curl u, the curl-flux estimate with
    mu = 1, Doerfler marking at 0.7, local refinement, solve on the constrained space, ESTIMATE ON THE REFINED MESH (B = R_rt C P_nd
    u in the constrained RT space, H its recovery in the constrained Nedelec space), mark, refine again, solve, estimate.
    The same loop through the CPU oracle (scipy P, the oracle's local operators, direct solves) gives the totals sqrt(sum eta_e^2)
        2.447304e-01 (80 elements), 1.542298e-01 (234 elements, 44 master faces), 7.517089e-02 (591 elements, 69 master faces)
    with 22 and 51 elements marked (the closures add none): the total falls from step to step, so that is asserted here."""
    from palace_amd.fem import nchex, rthex
    from palace_amd.fem.fespace import NDHexSpace
    from tests.test_nc_solve_gpu import _solve

    p = 2
    mesh = nu.start_mesh("C")
    totals, sizes = [], []
    for step in range(3):
        nd, rt = nchex.NCSpace(NDHexSpace(mesh, p)), nchex.NCSpace(rthex.RTHexSpace(mesh, p))
        conf = linalg.Conforming(ctx, nd)
        x, st, keep = _solve(ctx, nd, conf)
        assert st["converged"], (step, st)
        Bf = linalg.Curl(ctx, nd, rt, conforming=conf).mult(x, _new(rt.n_true))
        est, _, its = NCEstimator(ctx, nd, rt, "curl", [np.eye(3)]).estimate(Bf.cpu().numpy())
        assert np.all(np.isfinite(est)) and est.min() > 0.0
        totals.append(float(np.sqrt(est.sum())))
        sizes.append(mesh.ne)
        print(f"step {step}: {mesh.ne} elements, {nd.n_true} / {nd.n_local} Nedelec dofs, solve {st['iterations']} iterations, "
              f"projector {its}, total estimate {totals[-1]:.6e}")
        if step == 2:
            break
        marked = nchex.dorfler_mark(np.sqrt(est), 0.7)
        assert 0 < marked.size < mesh.ne
        mesh = nchex.refine_local(mesh, marked)
        assert mesh.master_faces.size > 0 and set(marked.tolist()) <= set(mesh.marked.tolist())
        assert _one_irregular(mesh)
    assert mesh.level.max() == 2          # the second closure refined children of the first step
    assert sizes[0] < sizes[1] < sizes[2]
    assert totals[0] > totals[1] > totals[2] > 0.0
