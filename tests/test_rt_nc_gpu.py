"""Raviart-Thomas spaces with hanging-face constraints on the device: the discrete curl between constrained spaces
(pa_curl_create_conforming: R_rt C_loc P_nd and its transpose) against scipy, ParOperator over the RT mass and over div-div + mass
with the RT constraint against the oracle with a scipy P and against the matrix of parallel_assemble, and Jacobi-PCG on P^T M P
(the gates of test_nc_solve_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import rt_nc_util as rn  # noqa: E402
from tests import rthex_util as ru  # noqa: E402
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


@pytest.mark.parametrize("name,p", [("A", 1), ("A", 2), ("A", 3), ("A", 5), ("C", 2)])
def test_curl_with_constraints(ctx, name, p):
    """R_rt C_loc P_nd on true-dof vectors and P_nd^T C_loc^T R_rt^T (zero-filled tail), relative error <= 1e-12."""
    nd, rt = nu.nc_space(name, "nd", p), rn.rt_space(name, p)
    Cu = linalg.Curl(ctx, nd, rt, conforming=linalg.Conforming(ctx, nd))
    Cl, Pn = rn.local_curl(nd, rt), nd.prolongation()
    rng = np.random.default_rng(30 + p)
    xn, xr = rng.uniform(-1, 1, nd.n_true), rng.uniform(-1, 1, rt.n_true)
    ref = (Cl @ (Pn @ xn))[: rt.n_true]
    got = Cu.mult(_dev(xn), _new(rt.n_true)).cpu().numpy()
    reft = Pn.T @ (Cl.T @ np.concatenate([xr, np.zeros(rt.n_local - rt.n_true)]))
    gott = Cu.mult_transpose(_dev(xr), _new(nd.n_true)).cpu().numpy()
    print(f"{name} p={p}: mult {_rel(got, ref):.2e} transpose {_rel(gott, reft):.2e}")
    assert _rel(got, ref) <= 1e-12 and _rel(gott, reft) <= 1e-12
    assert abs(xr @ got - xn @ gott) <= 1e-12 * abs(xr @ got)
    # the flux of a conforming field is conforming: the constrained tail of the local curl is what P_rt makes of the head
    assert _rel(rt.prolongation() @ got, Cl @ (Pn @ xn)) <= 1e-12


def test_curl_halo_and_constraint_together_are_refused(ctx):
    nd, rt = nu.nc_space("A", "nd", 1), rn.rt_space("A", 1)
    with pytest.raises(ValueError, match="together"):
        linalg.Curl(ctx, nd, rt, nd_halo=object(), conforming=object())


_FORMS = ("mass", "divdivmass")


def _rt_pair(ctx, name, p, form):
    """(space, local device operator, ParOperator with the RT constraint, its oracle, the oracle's local operator, keep-alive)."""
    rt = rn.rt_space(name, p)
    q1d = p + 1
    geom = _geom(rt.mesh, q1d)
    blob = util.make_ctx("aniso", 2)[1]
    if form == "mass":
        local = ceed.rtmass_operator(geom, rt, blob)
    elif form == "divdiv":
        local = ceed.divdiv_operator(geom, rt, ru.div_ctx().pack())
    else:
        local = ceed.divdivmass_operator(geom, rt, blob, ru.div_ctx().pack())
    conf = linalg.Conforming(ctx, rt)
    A = linalg.ParOperator(ctx, local, [], linalg.DIAG_ONE, conforming=conf)
    ol = rn.oracle_rt_local(rt, form)
    oA = nu.ConstrainedParOperatorOracle([ol], rt.prolongation(), [])
    return rt, local, A, oA, ol, conf


@pytest.mark.parametrize("form", ("mass", "divdiv", "divdivmass"))
@pytest.mark.parametrize("name,p", [("A", 1), ("A", 3), ("C", 2)])
def test_par_operator(ctx, name, p, form):
    """Mult, MultTranspose, AddMult, the diagonal |P|^T diag(A) and y = x in place against the oracle with a scipy P: 1e-12."""
    rt, local, A, oA, ol, conf = _rt_pair(ctx, name, p, form)
    n = rt.n_true
    assert A.n == n
    rng = np.random.default_rng(40 + p)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    ref = oA.mult(x)
    err = {}
    err["mult"] = _rel(A.mult(_dev(x), _new(n)).cpu().numpy(), ref)
    err["mult_transpose"] = _rel(A.mult_transpose(_dev(x), _new(n)).cpu().numpy(), ref)
    err["add_mult"] = _rel(A.add_mult(_dev(x), _dev(y0.copy()), -0.5).cpu().numpy(), oA.add_mult(x, y0, -0.5))
    err["diagonal"] = _rel(A.assemble_diagonal(_new(n)).cpu().numpy(), oA.diagonal())
    xy = _dev(x.copy())
    err["in_place"] = _rel(A.mult(xy, xy).cpu().numpy(), ref)
    print(" ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert max(err.values()) < 1e-12, err


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("name,p", [("A", 2), ("C", 1)])
def test_parallel_assemble(ctx, name, p, form):
    """The matrix of parallel_assemble is P^T A P (scipy, from the oracle's local matrix) and applies like the matrix-free
    operator, to 1e-12 of the largest entry."""
    rt, local, A, oA, ol, conf = _rt_pair(ctx, name, p, form)
    P = rt.prolongation()
    T = A.parallel_assemble()
    assert (T.nrows, T.ncols) == (rt.n_true, rt.n_true)
    Ts = T.to_scipy()
    ref = (P.T @ ol.assemble_sparse().tocsr() @ P).tocsr()
    d = abs(Ts - ref)
    assert (d.max() if d.nnz else 0.0) < 1e-12 * abs(ref).max()
    x = np.random.default_rng(50 + p).uniform(-1, 1, rt.n_true)
    y_free = A.mult(_dev(x), _new(rt.n_true)).cpu().numpy()
    y_asm = linalg.AssembledParOperator(ctx, T, [], linalg.DIAG_ONE).mult(_dev(x), _new(rt.n_true)).cpu().numpy()
    assert np.max(np.abs(y_asm - y_free)) < 1e-12 * np.max(np.abs(y_free))


@pytest.mark.parametrize("form", _FORMS)
def test_pcg_jacobi_matches_oracle(ctx, form):
    """Mesh C, order 2: iteration count +-1 and solution 1e-6 against oracle.pcg on the assembled P^T A P with the oracle's
    |P|^T diag (the gates of test_nc_solve_gpu.py::test_pcg_jacobi_matches_oracle)."""
    rt, local, A, oA, ol, conf = _rt_pair(ctx, "C", 2, form)
    n = rt.n_true
    P = rt.prolongation()
    PAP = (P.T @ ol.assemble_sparse().tocsr() @ P).tocsr()
    x0 = np.random.default_rng(12).uniform(-1, 1, n)
    assert _rel(PAP @ x0, oA.mult(x0)) < 1e-12
    b = oA.mult(np.ones(n))
    K = linalg.cg(ctx, A, linalg.jacobi(ctx, A), rel_tol=1e-8, max_it=500)
    x = K.mult(_dev(b), _new(n)).cpu().numpy()
    dinv = 1.0 / oA.diagonal()
    xo, it, hist = po.pcg(lambda v: PAP @ v, b, lambda r: dinv * r, rel_tol=1e-8, max_it=500)
    st = K.stats()
    print(st, it)
    assert st["converged"] and abs(st["iterations"] - it) <= 1
    assert _rel(x, xo) < 1e-6
    assert np.linalg.norm(oA.mult(x) - b) < 1e-6 * np.linalg.norm(b)
