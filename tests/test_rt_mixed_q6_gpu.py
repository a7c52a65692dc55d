"""Order 5 after the solve: the Raviart-Thomas operators and the two-space forms on hexahedra at six points per direction
(palace_amd/csrc/pa_rt_hex_q6.hip, pa_mixed_hex_q6.hip), every pair (1 ... 5, 6) of PA_HEX_Q6_LIST -- against the oracle,
through the estimator procedure for real and complex fields, and through the chain discrete curl -> curl-flux estimator.  The
meshes, materials and helpers are those of tests/test_rt_hex_gpu.py, tests/test_mixed_hex_gpu.py and
tests/test_two_part_hex_gpu.py (tests/rthex_util.py: at six points ogrid15 leaves the fourth workgroup with three live waves,
cyl80 gives 20 whole workgroups and, through test_mixed_hex_gpu._mesh, an internal element order that differs from the
caller's; every element rotated, two attributes)."""
import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import curl_util as cu
from tests import rthex_util as ru
from tests import test_mixed_hex_gpu as mh
from tests import test_rt_hex_gpu as rh
from tests import test_two_part_hex_gpu as tp
from tests import util

pytestmark = pytest.mark.gpu

Q1D = 6
Q6 = [(1, 6), (2, 6), (3, 6), (4, 6), (5, 6)]  # PA_HEX_Q6_LIST
CASES = [("ogrid15", p) for p, _ in Q6] + [("cyl80", 5)]  # every pair on the partial workgroup, order 5 on whole ones
REL = 1e-12  # the project's operator-level tolerance
_cache = {}


def _new(n, fill):
    import torch

    return torch.full((n,), fill, dtype=torch.float64, device="cuda")


# ---- Raviart-Thomas operators ------------------------------------------------------------------------

@pytest.mark.parametrize("qdata", ["packed", "matrixfree"])
@pytest.mark.parametrize("form", rh.FORMS)
@pytest.mark.parametrize("kind,p", CASES)
def test_rt_parity(monkeypatch, kind, p, form, qdata):
    """mult into a poisoned y, add_mult onto a non-zero y and (15-element mesh) the diagonal, for both D forms."""
    if qdata == "matrixfree":
        monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    op = rh._operator(kind, p, Q1D, form)
    x, ref = ru.oracle_mult(kind, p, Q1D, form)
    assert op.is_symmetric() and op.height == x.size
    y = _new(x.size, float("nan"))
    op.mult(rh._dev(x), y)
    e = rh._relerr(y.cpu().numpy(), ref)
    print(f"mult {e:.2e}")
    assert e < REL
    y0 = ru.vector(x.size, 5)
    y = rh._dev(y0)
    op.add_mult(rh._dev(x), y)
    e = np.abs(y.cpu().numpy() - (y0 + ref)).max() / np.abs(ref).max()
    print(f"add_mult {e:.2e}")
    assert e < REL
    if kind == "ogrid15":
        d = _new(x.size, 3.0)
        op.assemble_diagonal(d)
        e = rh._relerr(d.cpu().numpy(), ru.oracle_diag(kind, p, Q1D, form))
        print(f"diagonal {e:.2e}")
        assert e < REL


@pytest.mark.parametrize("kind,p", CASES)
def test_rt_transpose_of_a_nonsymmetric_mass(kind, p):
    """A general 3 x 3 material (matrix-free D): A^T is the oracle's operator with every material matrix transposed."""
    op = rh._operator(kind, p, Q1D, "mass", mass="nonsym")
    assert not op.is_symmetric()
    z = ru.vector(op.height, 17)
    _, ref = ru.oracle_mult(kind, p, Q1D, "mass", mass="nonsym", x=z)
    _, tref = ru.oracle_mult(kind, p, Q1D, "mass", mass="nonsym_t", x=z)
    assert rh._relerr(ref, tref) > 1e-3  # the two operators really differ
    assert rh._relerr(rh._mult(op, z), ref) < REL
    atz = _new(z.size, float("nan"))
    op.mult_transpose(rh._dev(z), atz)
    e = rh._relerr(atz.cpu().numpy(), tref)
    print(f"mult_transpose {e:.2e}")
    assert e < REL


@pytest.mark.parametrize("qdata", ["packed", "matrixfree"])
@pytest.mark.parametrize("kind,p", CASES)
def test_rt_essential_dofs(monkeypatch, kind, p, qdata):
    """ParOperator with the boundary-face dofs essential, both diagonal policies: entries read as zero, rows fixed."""
    from palace_amd import linalg

    if qdata == "matrixfree":
        monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    form = "divdivmass"
    op = rh._operator(kind, p, Q1D, form)
    ess = ru.boundary_dofs(kind, p)
    assert 0 < ess.size < op.height
    x = ru.vector(op.height, 23)
    tx = x.copy()
    tx[ess] = 0.0
    _, ref0 = ru.oracle_mult(kind, p, Q1D, form, x=tx)
    scale = np.abs(ref0).max()
    ctx = linalg.Context()
    for policy, diag in (("one", linalg.DIAG_ONE), ("zero", linalg.DIAG_ZERO)):
        A = linalg.ParOperator(ctx, op, ess, diag)
        ref = ref0.copy()
        ref[ess] = x[ess] if policy == "one" else 0.0
        y = _new(x.size, 7.0)
        A.mult(rh._dev(x), y)
        e = np.abs(y.cpu().numpy() - ref).max() / scale
        print(f"policy {policy}: {e:.2e}")
        assert e < REL


@pytest.mark.parametrize("p", [1, 5])
def test_rt_full_assembly(p):
    """The coarsest and the finest level of an order-5 Raviart-Thomas hierarchy, assembled by probing through the apply."""
    kind, form = "ogrid15", "divdivmass"
    op = rh._operator(kind, p, Q1D, form)
    A = op.full_assemble()
    x, ref = ru.oracle_mult(kind, p, Q1D, form)
    ax = rh._mult(op, x)
    assert rh._relerr(A @ x, ax) < REL and rh._relerr(ax, ref) < REL
    assert abs(A - A.T).max() < 1e-12 * abs(A).max()


# ---- two-space forms ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nd_trial", [True, False], ids=["hcurlhdiv", "hdivhcurl"])
@pytest.mark.parametrize("kind,p", CASES)
def test_mixed_mass(kind, p, nd_trial):
    """mult, add_mult onto a non-zero y and mult_transpose with a non-symmetric material: A against the oracle, A^T against
    the oracle's operator of the other QFunction with every material matrix transposed."""
    op = mh._mass_operator(kind, p, Q1D, nd_trial)
    assert not op.is_symmetric()
    x, ref = mh._mass_reference(kind, p, Q1D, nd_trial, "nonsym")
    y = _new(op.height, float("nan"))
    op.mult(mh._dev(x), y)
    e = mh._relerr(y.cpu().numpy(), ref)
    print(f"mult {e:.2e}")
    assert e < REL
    y0 = ru.vector(ref.size, 5)
    y = mh._dev(y0)
    op.add_mult(mh._dev(x), y)
    e = np.abs(y.cpu().numpy() - (y0 + ref)).max() / np.abs(ref).max()
    print(f"add_mult {e:.2e}")
    assert e < REL
    z, tref = mh._mass_reference(kind, p, Q1D, not nd_trial, "nonsym_t")  # maps the test space of `op` to its trial space
    assert z.size == op.height and tref.size == op.width
    e = mh._relerr(mh._mult(op, z, transpose=True), tref)
    print(f"mult_transpose {e:.2e}")
    assert e < REL


@pytest.mark.parametrize("nd_first", [True, False], ids=["hcurlhdiv_error", "hdivhcurl_error"])
@pytest.mark.parametrize("kind,p", CASES)
def test_element_error(kind, p, nd_first):
    """ApplyAdd into a non-zero estimate vector against the oracle; the estimates are in the caller's element order although
    the kernel walks the geometry data's own; a second run gives the same bits."""
    geom = mh._geom(kind, Q1D)
    if kind == "cyl80":
        assert not np.array_equal(mh._element_order(geom), np.arange(geom.mesh.ne))
    (s1, o1), (s2, o2) = mh._sides(kind, p, Q1D, nd_first)
    c_an, _ = util.make_ctx("aniso", 2)
    c_ns, _ = util.make_ctx("nonsym", 2)
    qfo = po.QF_HCURLHDIV_ERROR if nd_first else po.QF_HDIVHCURL_ERROR
    integ = tp._error_integrator(kind, p, Q1D, nd_first)
    rng = np.random.default_rng(10 * p + Q1D)
    u1, u2 = rng.uniform(-1, 1, s1.ndofs), rng.uniform(-1, 1, s2.ndofs)
    e0 = rng.uniform(0, 1, integ.ne)
    ref = po.MixedSpaceOracle(o1, o2, mh._ogeom(kind, Q1D), qfo, c_an, c_ns).error_add(u1, u2, e0.copy())
    d1, d2 = mh._dev(u1), mh._dev(u2)
    est = integ.apply_add(d1, d2, mh._dev(e0.copy())).cpu().numpy()
    e = mh._relerr(est, ref)
    print(f"error {e:.2e}")
    assert e < REL
    assert (ref - e0).min() > 0
    assert np.array_equal(est, integ.apply_add(d1, d2, mh._dev(e0.copy())).cpu().numpy())


def test_ragged_tail_of_workgroups():
    """270 elements: 68 workgroups of four waves, the last one half full; if the kernels deal workgroups to the eight XCDs in
    chunks (9 per XCD, 72 launched) the last ones lie past the end.  Order 5: the RT mass and the error integrator."""
    from palace_amd import ceed
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.fem.mesh import ogrid_cylinder

    p = 5
    mesh = ogrid_cylinder(3, 6)
    assert mesh.ne == 270
    nd, sp = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p)
    geom, og = ceed.GeomFactorData(mesh, Q1D), util.oracle_geom(mesh, Q1D)
    c_an, b_an = util.make_ctx("aniso", 2)
    c_ns, b_ns = util.make_ctx("nonsym", 2)
    rint, _ = ru.tables(p, Q1D)
    rto = po.CeedOperatorOracle(sp.ndofs, sp.elem_dof_lex, sp.elem_sign_lex < 0, rint, rint, og, po.QF_HDIV, c_an)
    x = ru.vector(sp.ndofs, 8)
    y = rh._mult(ceed.rtmass_operator(geom, sp, b_an), x)
    e = rh._relerr(y, rto.apply_add(x, np.zeros(sp.ndofs)))
    print(f"RT mass {e:.2e}")
    assert e < REL
    off, ori = nd.native_restriction()
    nint, ncurl = util.dense_tables(nd, Q1D)
    nint, ncurl = np.asarray(nint).reshape(3, -1, nd.P), np.asarray(ncurl).reshape(3, -1, nd.P)
    ndo = po.CeedOperatorOracle(nd.ndofs, off, ori, nint, ncurl, og, po.QF_HCURL, None)
    integ = ceed.HexElementErrorIntegrator(geom, nd, sp, ceed.QF_HCURLHDIV_ERROR_33, np.concatenate([b_an, b_ns]))
    assert integ.ne == mesh.ne
    u1, u2 = ru.vector(nd.ndofs, 9), ru.vector(sp.ndofs, 10)
    e0 = np.random.default_rng(11).uniform(0, 1, mesh.ne)
    ref = po.MixedSpaceOracle(ndo, rto, og, po.QF_HCURLHDIV_ERROR, c_an, c_ns).error_add(u1, u2, e0.copy())
    est = integ.apply_add(mh._dev(u1), mh._dev(u2), mh._dev(e0.copy())).cpu().numpy()
    e = mh._relerr(est, ref)
    print(f"error {e:.2e}")
    assert e < REL and (ref - e0).min() > 0


# ---- the estimator procedure at order 5 --------------------------------------------------------------

@pytest.mark.parametrize("direction", ["grad", "curl"])
def test_flux_error_estimate_at_order_five(direction):
    """test_mixed_hex_gpu.test_flux_error_estimate at the order its dense solve still reaches on 15 elements."""
    est, D, est_o, D_o, _ = mh._estimate(5, direction)
    eD, ee = mh._relerr(D, D_o), np.abs(est - est_o).max() / est_o.max()
    print(f"smooth flux {eD:.2e} estimates {ee:.2e}")
    assert eD < 1e-9 and ee < 1e-9
    assert est_o.min() > 0 and est.min() > 0


def test_two_part_queries_answer_no_at_six_points():
    """No both-parts-per-pass kernel at six points: mult2 and apply_add2 are two one-part passes."""
    kind, p = "ogrid15", 5
    assert (p, Q1D) not in tp.MIXED2 and (p, Q1D) not in tp.ERROR2 and (p, Q1D) not in tp.RT2
    flux, rt = mh._mass_operator(kind, p, Q1D, True), rh._operator(kind, p, Q1D, "mass")
    integ = tp._error_integrator(kind, p, Q1D, True)
    assert not flux.two_rhs() and not rt.two_rhs() and not integ.two_parts()
    for op in (flux, rt):
        x0, x1 = ru.vector(op.width, 1), ru.vector(op.width, 2)
        y0, y1 = tp._mult2(op, x0, x1)
        assert np.array_equal(y0, mh._mult(op, x0)) and np.array_equal(y1, mh._mult(op, x1))
    (s1, _), (s2, _) = mh._sides(kind, p, Q1D, True)
    dev = [mh._dev(ru.vector(m, s)) for m, s in ((s1.ndofs, 5), (s2.ndofs, 6), (s1.ndofs, 7), (s2.ndofs, 8))]
    start = np.random.default_rng(3).uniform(0, 1, integ.ne)
    est = integ.apply_add2(*dev, mh._dev(start.copy())).cpu().numpy()
    two = mh._dev(start.copy())
    integ.apply_add(dev[0], dev[1], two)
    integ.apply_add(dev[2], dev[3], two)
    assert np.array_equal(est, two.cpu().numpy()) and (est - start).min() > 0


@pytest.mark.parametrize("direction", ["grad", "curl"])
def test_complex_flux_error_estimate_at_order_five(direction):
    """test_two_part_hex_gpu.test_complex_flux_error_estimate (complex_device_estimate against the oracle run on each part)
    on the two-pass fall-back."""
    tp.test_complex_flux_error_estimate(5, direction)


def _oracle_curl_estimate(field):
    """The oracle procedure of test_mixed_hex_gpu._estimate, direction "curl", for a given flux density in the RT space."""
    kind, p = "ogrid15", 5
    (s1, o1), (s2, o2) = mh._sides(kind, p, Q1D, False)
    c_mat, c_sq, c_isq = mh.estimator_materials()
    og = mh._ogeom(kind, Q1D)
    Mo = po.CeedOperatorOracle(o2.lsize, o2.off, o2.sgn < 0, o2.interp, o2.interp, og, po.QF_HCURL, po.CoeffCtx())
    rhs_o = po.MixedSpaceOracle(o1, o2, og, po.QF_HDIVHCURL, c_mat).apply_add(field, np.zeros(s2.ndofs))
    H_o = np.linalg.solve(Mo.assemble_sparse().toarray(), rhs_o)
    return po.MixedSpaceOracle(o1, o2, og, po.QF_HDIVHCURL_ERROR, c_sq, c_isq).error_add(field, H_o, np.zeros(o1.NE)), H_o


def test_curl_then_estimate_at_order_five():
    """What a user runs after an order-5 solve: B = curl A by the discrete curl, then the curl-flux estimator on B."""
    from palace_amd import linalg

    kind, p = "ogrid15", 5
    nd, rt = cu.spaces(kind, p)
    assert mh._mesh(kind) is ru.mesh(kind)
    A = ru.vector(nd.ndofs, 41)
    B = linalg.Curl(linalg.Context(), nd, rt).mult(mh._dev(A), _new(rt.ndofs, float("nan"))).cpu().numpy()
    B_o = cu.oracle(kind, p).mult(A)
    assert mh._relerr(B, B_o) < 1e-13
    est, H, _ = mh.device_estimate(ru.mesh(kind), p, "curl", B)
    est_o, H_o = _oracle_curl_estimate(B_o)
    eH, ee = mh._relerr(H, H_o), np.abs(est - est_o).max() / est_o.max()
    print(f"smooth flux {eH:.2e} estimates {ee:.2e}")
    assert eH < 1e-9 and ee < 1e-9
    assert est_o.min() > 0 and est.min() > 0


# ---- refusals unchanged ------------------------------------------------------------------------------

def test_refusals_unchanged():
    from palace_amd import ceed
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.lib import PalaceAmdError

    kind = "ogrid15"
    mesh = ru.mesh(kind)
    _, blob = util.make_ctx("aniso", 2)
    nd4, sp4 = mh._spaces(kind, 4)
    with pytest.raises(PalaceAmdError, match=r"no H\(div\) hex kernel for order 4 with 4 points"):
        ceed.rtmass_operator(mh._geom(kind, 4), sp4, blob)
    with pytest.raises(PalaceAmdError, match=r"no H\(curl\) - H\(div\) hex kernel for order 4 with 4 points"):
        ceed.mixedmass_operator(mh._geom(kind, 4), nd4, sp4, blob)
    with pytest.raises(PalaceAmdError, match=r"no H\(curl\) - H\(div\) hex kernel for order 4 with 4 points"):
        ceed.HexElementErrorIntegrator(mh._geom(kind, 4), nd4, sp4, ceed.QF_HCURLHDIV_ERROR_33, np.concatenate([blob, blob]))
    geom7 = ceed.GeomFactorData(mesh, 7)
    with pytest.raises(PalaceAmdError, match=r"no H\(div\) hex kernel for order 6 with 7 points"):
        ceed.rtmass_operator(geom7, rthex.RTHexSpace(mesh, 6), blob)
    with pytest.raises(PalaceAmdError, match=r"no H\(curl\) - H\(div\) hex kernel for order 6 with 7 points"):
        ceed.mixedmass_operator(geom7, NDHexSpace(mesh, 6), rthex.RTHexSpace(mesh, 6), blob)
