"""Order-5 hexahedra: the H(curl) and H1 element kernels at six points per direction (palace_amd/csrc/pa_nd_hex_q6.hip,
pa_h1_hex_q6.hip; the pairs of PA_HEX_Q6_LIST) and everything above them -- coarsening, diagonal, essential dofs, transpose,
full assembly, p-multigrid, the complex wrapper -- through the C ABI against the oracle, on the two rotated meshes of
tests/rthex_util.py.  Criterion of tests/test_apply_gpu.py: relative L2 error below 1e-12.

The oracle's references are computed once per (mesh, order, form, coefficient) and shared by the variants of a case; the
order-5 diagonal of the numpy oracle (element matrices) is the slow part: 1.5-3 s per case on the 15-element mesh, 8-16 s for
each of the three cases on the 80-element mesh (measured), all of it on the CPU."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, lib, linalg  # noqa: E402
from tests import rthex_util as ru  # noqa: E402
from tests import transfer_util as tu  # noqa: E402
from tests import util  # noqa: E402

RTOL = 1e-12
Q1D = 6
# every (p, q1d) pair of PA_HEX_Q6_LIST, for both families (tests/test_hex_q6_host.py compares)
ND_PQ = [(1, 6), (2, 6), (3, 6), (4, 6), (5, 6)]
H1_PQ = [(1, 6), (2, 6), (3, 6), (4, 6), (5, 6)]
VARIANTS = ["default", "matrix_free", "nonsym", "iso_matrix_free", "atomic", "metric", "iso_qdata"]
COEF = {"default": "aniso", "matrix_free": "aniso", "nonsym": "nonsym", "iso_matrix_free": "scalar", "atomic": "aniso",
        "metric": "scalar", "iso_qdata": "scalar"}
ND_CASES = [("ogrid15", p, v) for p, _ in ND_PQ for v in VARIANTS] + [("cyl80", 5, "default")]
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.empty(n, dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _geom(kind):
    if ("geom", kind) not in _cache:
        _cache["geom", kind] = ceed.GeomFactorData(ru.mesh(kind), Q1D)
    return _cache["geom", kind]


def _ctx(coef, transposed=False):
    """(oracle context, blob) of a two-attribute coefficient; transposed: every material matrix transposed."""
    if coef == "nonsym" and transposed:
        c = ru.mass_ctx("nonsym_t")
        return c, c.pack()
    return util.make_ctx(coef, 2)


def _nd_operator(kind, p, qf, coef):
    nd, geom = tu.space(kind, "nd", p), _geom(kind)
    _, b_a = _ctx(coef)
    _, b_s = _ctx("scalar")
    if qf == "hdiv":
        return ceed.curlcurl_operator(geom, nd, b_a)
    if qf == "hcurl":
        return ceed.ndmass_operator(geom, nd, b_a)
    return ceed.curlcurlmass_operator(geom, nd, b_s, b_a)


def _nd_blob(qf, coef, transposed=False):
    _, b_a = _ctx(coef, transposed)
    return b_a if qf != "hdivmass" else np.concatenate([_ctx("scalar")[1], b_a])


def _nd_ref(kind, p, qf, coef, transposed=False):
    """(x, A x) -- or A^T x -- through the C oracle, the input fixed per (order, form)."""
    key = ("ndref", kind, p, qf, coef, transposed)
    if key not in _cache:
        nd = tu.space(kind, "nd", p)
        x = ru.vector(nd.ndofs, 60 + 7 * p + len(qf))
        _cache[key] = (x, util.oracle_apply_c(nd, ru.ogeom(kind, Q1D), qf, _nd_blob(qf, coef, transposed), x, Q1D))
    return _cache[key]


def _nd_diag(kind, p, qf, coef):
    key = ("nddiag", kind, p, qf, coef)
    if key not in _cache:
        c_a, c_s = _ctx(coef)[0], _ctx("scalar")[0]
        args = (c_s, c_a) if qf == "hdivmass" else (c_a, None)
        _cache[key] = util.oracle_operator(tu.space(kind, "nd", p), ru.ogeom(kind, Q1D), qf, *args, Q1D).diagonal()
    return _cache[key]


@pytest.mark.parametrize("kind", ru.MESHES)
def test_geometry_factors_at_six_points(kind):
    g = _geom(kind).to_numpy()
    ref = ru.ogeom(kind, Q1D)
    assert np.array_equal(g[:, 0, :], ref[:, 0, :])
    np.testing.assert_allclose(g[:, 1:, :], ref[:, 1:, :], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("qf", ["hdiv", "hcurl", "hdivmass"])
@pytest.mark.parametrize("kind,p,variant", ND_CASES)
def test_nd_apply_add_mult_and_diagonal(monkeypatch, kind, p, variant, qf):
    """Every D stage and both forms of E^T of the six-point H(curl) kernel: Mult, AddMult accumulating, the diagonal; for
    the non-symmetric coefficient also MultTranspose (the operator with every material matrix transposed)."""
    if variant in ("matrix_free", "iso_matrix_free"):
        monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    if variant == "atomic":
        monkeypatch.setenv("PALACE_AMD_SCATTER", "atomic")
    if variant == "metric":
        monkeypatch.setenv("PALACE_AMD_DSTAGE", "metric")
    if variant == "iso_qdata":
        monkeypatch.setenv("PALACE_AMD_DSTAGE", "qdata")
    coef = COEF[variant]
    op = _nd_operator(kind, p, qf, coef)
    n = op.height
    x, ref = _nd_ref(kind, p, qf, coef)
    y = op.mult(_dev(x), _new(n)).cpu().numpy()
    print(f"mult {_rel(y, ref):.2e}")
    assert _rel(y, ref) < RTOL
    y2 = op.add_mult(_dev(x), _dev(ref.copy())).cpu().numpy()
    print(f"add_mult {_rel(y2, 2 * ref):.2e}")
    assert _rel(y2, 2 * ref) < RTOL
    d = op.assemble_diagonal(_new(n)).cpu().numpy()
    dref = _nd_diag(kind, p, qf, coef)
    print(f"diagonal {_rel(d, dref):.2e}")
    assert _rel(d, dref) < RTOL
    if variant == "nonsym":
        assert not op.is_symmetric()
        _, ref_t = _nd_ref(kind, p, qf, coef, transposed=True)
        yt = op.mult_transpose(_dev(x), _new(n)).cpu().numpy()
        print(f"mult_transpose {_rel(yt, ref_t):.2e}")
        assert _rel(yt, ref_t) < RTOL and _rel(ref_t, ref) > 1e-3


@pytest.mark.parametrize("p", [5, 2])
def test_mixed_curl_forms(p):
    """(C u, curl v) and (C curl u, v) on one H(curl) space with a general coefficient: each form and its transpose (the
    other form with C transposed)."""
    kind = "ogrid15"
    nd, geom, ogeom = tu.space(kind, "nd", p), _geom(kind), ru.ogeom(kind, Q1D)
    c, blob = _ctx("nonsym")
    ct, _ = _ctx("nonsym", transposed=True)
    x = ru.vector(nd.ndofs, 31 + p)
    for form, other, build in (("hcurlhdiv", "hdivhcurl", ceed.weakcurl_operator), ("hdivhcurl", "hcurlhdiv", ceed.mixedcurl_operator)):
        op = build(geom, nd, blob)
        ref = util.oracle_operator(nd, ogeom, form, c, None, Q1D).apply_add(x, np.zeros(nd.ndofs))
        assert np.linalg.norm(ref) > 1e-3
        assert _rel(op.mult(_dev(x), _new(nd.ndofs)).cpu().numpy(), ref) < RTOL, form
        ref_t = util.oracle_operator(nd, ogeom, other, ct, None, Q1D).apply_add(x, np.zeros(nd.ndofs))
        assert _rel(op.mult_transpose(_dev(x), _new(nd.ndofs)).cpu().numpy(), ref_t) < RTOL, (form, "T")


@pytest.mark.parametrize("p", [5, 1])
@pytest.mark.parametrize("policy", ["one", "zero"])
def test_essential_dofs(p, policy):
    """pa_op_mult_essential_diag (rows fixed by the caller where the kernels do not) and ParOperator.mult against the
    oracle's ParOperator."""
    kind = "ogrid15"
    nd = tu.space(kind, "nd", p)
    ess = nd.ess_dofs()
    assert 0 < ess.size < nd.ndofs
    cs, bs = _ctx("scalar")
    ca, ba = _ctx("aniso")
    op = _nd_operator(kind, p, "hdivmass", "aniso")
    orc = util.FastParOperatorOracle(nd, ru.ogeom(kind, Q1D), "hdivmass", np.concatenate([bs, ba]), ess, Q1D, cs, ca,
                                     policy=po.DIAG_ONE if policy == "one" else po.DIAG_ZERO)
    x = ru.vector(nd.ndofs, 17 + p)
    ref = orc.mult(x)
    A = linalg.ParOperator(linalg.Context(), op, ess, linalg.DIAG_ONE if policy == "one" else linalg.DIAG_ZERO)
    y = torch.full((nd.ndofs,), 7.0, dtype=torch.float64, device="cuda")
    A.mult(_dev(x), y)
    assert _rel(y.cpu().numpy(), ref) < RTOL
    handled = C.c_int(-1)
    y2 = torch.full((nd.ndofs,), 7.0, dtype=torch.float64, device="cuda")
    xd = _dev(x)
    lib.check(lib.load().pa_op_mult_essential_diag(op.handle, C.c_void_p(xd.data_ptr()), C.c_void_p(y2.data_ptr()),
                                                   C.c_int(1 if policy == "one" else 0), None, C.byref(handled)))
    torch.cuda.synchronize()
    y2 = y2.cpu().numpy()
    assert handled.value in (0, 1)
    if handled.value == 0:
        y2[ess] = x[ess] if policy == "one" else 0.0
    assert _rel(y2, ref) < RTOL
    d = A.assemble_diagonal(_new(nd.ndofs)).cpu().numpy()
    dref = _nd_diag(kind, p, "hdivmass", "aniso").copy()
    dref[ess] = 1.0 if policy == "one" else 0.0
    assert _rel(d, dref) < RTOL


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_coarsened_levels(p):
    """fine.coarsen(geom, space_p) is the operator built at (p, 6), and the oracle's."""
    kind = "ogrid15"
    if ("fine", kind) not in _cache:
        _cache["fine", kind] = _nd_operator(kind, 5, "hdivmass", "aniso")
    fine = _cache["fine", kind]
    nd = tu.space(kind, "nd", p)
    coarse = fine.coarsen(_geom(kind), nd)
    direct = _nd_operator(kind, p, "hdivmass", "aniso")
    x, ref = _nd_ref(kind, p, "hdivmass", "aniso")
    yc = coarse.mult(_dev(x), _new(nd.ndofs)).cpu().numpy()
    yd = direct.mult(_dev(x), _new(nd.ndofs)).cpu().numpy()
    assert _rel(yc, ref) < RTOL and _rel(yc, yd) < 1e-13
    assert not coarse.streams() and not coarse.two_rhs() and not coarse.supports_split()
    dc = coarse.assemble_diagonal(_new(nd.ndofs)).cpu().numpy()
    assert _rel(dc, _nd_diag(kind, p, "hdivmass", "aniso")) < RTOL


def _h1_ctxs():
    rng = np.random.default_rng(7)
    A = rng.uniform(-1, 1, (3, 3))
    spd = A @ A.T + 2.0 * np.eye(3)
    c_diff = po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[spd, np.array([0.7])], a=1.3)
    c_mass = po.CoeffCtx(attr_mat=[1, 0], mat_coeff=[np.array([2.08]), np.array([0.5])], dim=1)
    return c_mass, c_diff


def _h1_oracle(kind, p, qf):
    """(x, A x, diag A) of the numpy oracle."""
    key = ("h1ref", kind, p, qf)
    if key not in _cache:
        h1 = tu.space(kind, "h1", p)
        c_mass, c_diff = _h1_ctxs()
        interp, grad = po.h1_hex_dense_tables(p, Q1D)
        which = {"diffusion": (po.QF_HCURL, c_diff, None), "mass": (po.QF_H1MASS, c_mass, None),
                 "diffusionmass": (po.QF_HCURLMASS, c_mass, c_diff)}[qf]
        o = po.CeedOperatorOracle(h1.ndofs, h1.elem_dof_lex, None, interp, grad, ru.ogeom(kind, Q1D), *which, vector_fe=False)
        x = ru.vector(h1.ndofs, 90 + p)
        _cache[key] = (x, o.apply_add(x, np.zeros(h1.ndofs)), o.diagonal())
    return _cache[key]


def _h1_operator(kind, p, qf):
    h1, geom = tu.space(kind, "h1", p), _geom(kind)
    c_mass, c_diff = _h1_ctxs()
    if qf == "diffusion":
        return ceed.diffusion_operator(geom, h1, c_diff.pack())
    if qf == "mass":
        return ceed.h1mass_operator(geom, h1, c_mass.pack())
    return ceed.diffusionmass_operator(geom, h1, c_mass.pack(), c_diff.pack())


@pytest.mark.parametrize("p,q1d", H1_PQ)
@pytest.mark.parametrize("qf", ["diffusion", "mass", "diffusionmass"])
@pytest.mark.parametrize("dstage", ["qdata", "matrix_free"])
def test_h1_apply_and_diagonal(monkeypatch, p, q1d, qf, dstage):
    assert q1d == Q1D
    if dstage == "matrix_free":
        monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    op = _h1_operator("ogrid15", p, qf)
    x, ref, dref = _h1_oracle("ogrid15", p, qf)
    y = op.mult(_dev(x), _new(x.size)).cpu().numpy()
    print(f"mult {_rel(y, ref):.2e}")
    assert _rel(y, ref) < RTOL
    d = op.assemble_diagonal(_new(x.size)).cpu().numpy()
    assert _rel(d, dref) < RTOL


def test_bit_reproducible():
    """Two Mults of the same order-5 operator on the E-vector path (fixed summation order in the gather)."""
    op = _nd_operator("ogrid15", 5, "hdivmass", "aniso")
    x = _dev(ru.vector(op.height, 3))
    y0, y1 = op.mult(x, _new(op.height)), op.mult(x, _new(op.height))
    assert torch.equal(y0, y1) and float(y0.abs().max()) > 0


@pytest.mark.parametrize("family", ["nd", "h1"])
def test_full_assembly_on_the_coarsest_level(family):
    """The (1, 6) level of an order-5 hierarchy, assembled by probing through the apply: the CSR matrix reproduces Mult
    and its diagonal is assemble_diagonal."""
    kind = "ogrid15"
    sp = tu.space(kind, family, 1)
    fine = _nd_operator(kind, 5, "hdivmass", "aniso") if family == "nd" else _h1_operator(kind, 5, "diffusionmass")
    op = fine.coarsen(_geom(kind), sp)
    A = op.full_assemble()
    x = ru.vector(sp.ndofs, 5)
    y = op.mult(_dev(x), _new(sp.ndofs)).cpu().numpy()
    assert np.abs(A @ x - y).max() < 1e-12 * np.abs(y).max()
    d = op.assemble_diagonal(_new(sp.ndofs)).cpu().numpy()
    assert np.abs(A.diagonal() - d).max() < 1e-12 * np.abs(d).max()
    if family == "nd":
        ref = util.oracle_apply_c(sp, ru.ogeom(kind, Q1D), "hdivmass", _nd_blob("hdivmass", "aniso"), x, Q1D)
        assert _rel(A @ x, ref) < RTOL


def test_blocks_dealt_to_the_xcds_with_a_ragged_tail():
    """270 elements: 68 workgroups of four waves, dealt round-robin to the eight XCDs in chunks of 9 (72 launched, the
    last ones past the end, the last real one half full).  Order 2 so that the oracle stays short."""
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.fem.mesh import ogrid_cylinder

    mesh = ogrid_cylinder(3, 6)
    assert mesh.ne == 270
    nd = NDHexSpace(mesh, 2)
    geom = ceed.GeomFactorData(mesh, Q1D)
    _, b_s = util.make_ctx("scalar")
    _, b_a = util.make_ctx("aniso")
    op = ceed.curlcurlmass_operator(geom, nd, b_s, b_a)
    x = ru.vector(nd.ndofs, 8)
    y = op.mult(_dev(x), _new(nd.ndofs)).cpu().numpy()
    ref = util.oracle_apply_c(nd, util.oracle_geom(mesh, Q1D), "hdivmass", np.concatenate([b_s, b_a]), x, Q1D)
    assert _rel(y, ref) < RTOL


class Problem:
    """(K + M) on ogrid15 at orders `levels`, device and oracle side by side (as in tests/test_solvers_gpu.py)."""

    def __init__(self, kind, levels):
        mesh = ru.mesh(kind)
        self.levels, self.ctx, self.geom, self.ogeom = levels, linalg.Context(), _geom(kind), ru.ogeom(kind, Q1D)
        self.cm, self.bm = util.make_ctx("scalar", 2)
        self.cc, self.bc = util.make_ctx("identity")
        self.spaces = [tu.space(kind, "nd", p) for p in levels]
        assert mesh.ne == 15
        fine = ceed.curlcurlmass_operator(self.geom, self.spaces[-1], self.bm, self.bc)
        self.local = [fine.coarsen(self.geom, s) for s in self.spaces[:-1]] + [fine]
        self.A = [linalg.ParOperator(self.ctx, op, s.ess_dofs(), linalg.DIAG_ONE) for op, s in zip(self.local, self.spaces)]
        blob = np.concatenate([self.bm, self.bc])
        self.oA = [util.FastParOperatorOracle(s, self.ogeom, "hdivmass", blob, s.ess_dofs(), Q1D, self.cm, self.cc)
                   for s in self.spaces]
        self.P = [linalg.Interp(self.ctx, a, b) for a, b in zip(self.spaces[:-1], self.spaces[1:])]
        self.oP = [po.InterpOracle(a.elem_dof_lex, a.elem_sign_lex, b.elem_dof_lex, b.elem_sign_lex, a.ndofs, b.ndofs,
                                   po.nd_hex_interp_lex(a.p, b.p)) for a, b in zip(self.spaces[:-1], self.spaces[1:])]


@pytest.fixture(scope="module")
def prob():
    return Problem("ogrid15", [1, 3, 5])


def test_gmg_vcycle_and_pcg(prob):
    """One V-cycle (levels 1, 3, 5; 4th-kind Chebyshev of order 6; Jacobi-PCG coarse solve) against GMGOracle, then PCG +
    GMG: the oracle's iteration count +- 1 and its solution."""
    n = prob.spaces[-1].ndofs
    cs = linalg.cg(prob.ctx, prob.A[0], linalg.jacobi(prob.ctx, prob.A[0]), rel_tol=1e-3, max_it=200)
    B = linalg.gmg(prob.ctx, prob.A, prob.P, cs, cheby_order=6)
    lam = [linalg.chebyshev(prob.ctx, prob.A[l], order=6).lambda_max() for l in (1, 2)]
    sm = [None] + [po.ChebyshevOracle(prob.oA[l], 6, lambda_max=lam[l - 1]) for l in (1, 2)]
    d0 = 1.0 / prob.oA[0].diagonal()
    coarse = lambda r: po.pcg(prob.oA[0].mult, r, lambda v: d0 * v, rel_tol=1e-3, max_it=200)[0]  # noqa: E731
    oB = po.GMGOracle(prob.oA, [(p.mult, p.mult_transpose) for p in prob.oP], sm, coarse, [s.ess_dofs() for s in prob.spaces])
    r = ru.vector(n, 8)
    r[prob.spaces[-1].ess_dofs()] = 0.0
    z = B.mult(_dev(r), torch.zeros(n, dtype=torch.float64, device="cuda")).cpu().numpy()
    print(f"V-cycle {_rel(z, oB.mult(r)):.2e}")
    assert _rel(z, oB.mult(r)) < 1e-8
    b = prob.oA[-1].mult(np.ones(n))
    b[prob.spaces[-1].ess_dofs()] = 0.0
    K = linalg.cg(prob.ctx, prob.A[-1], B, rel_tol=1e-8, max_it=100)
    x = K.mult(_dev(b), torch.zeros(n, dtype=torch.float64, device="cuda")).cpu().numpy()
    xo, it, _ = po.pcg(prob.oA[-1].mult, b, oB.mult, rel_tol=1e-8, max_it=100)
    st = K.stats()
    print(f"PCG + GMG: {st['iterations']} iterations, oracle {it}")
    assert st["converged"] and abs(st["iterations"] - it) <= 1, (st, it)
    assert _rel(x, xo) < 1e-6


def test_pcg_jacobi(prob):
    n = prob.spaces[-1].ndofs
    b = prob.oA[-1].mult(np.ones(n))
    b[prob.spaces[-1].ess_dofs()] = 0.0
    K = linalg.cg(prob.ctx, prob.A[-1], linalg.jacobi(prob.ctx, prob.A[-1]), rel_tol=1e-8, max_it=600)
    x = K.mult(_dev(b), torch.zeros(n, dtype=torch.float64, device="cuda")).cpu().numpy()
    dinv = 1.0 / prob.oA[-1].diagonal()
    xo, it, _ = po.pcg(prob.oA[-1].mult, b, lambda r: dinv * r, rel_tol=1e-8, max_it=600)
    st = K.stats()
    print(f"Jacobi-PCG: {st['iterations']} iterations, oracle {it}")
    assert st["converged"] and abs(st["iterations"] - it) <= 1, (st, it)
    assert _rel(x, xo) < 1e-6


def test_complex_wrapper():
    """ComplexWrapperOperator of (K - w^2 M, w C) at order 5 -- separate applies: there is no one-pass complex form and no
    two-vector form at six points -- against four oracle applies."""
    kind, p, w = "ogrid15", 5, 0.8
    nd, geom, ogeom = tu.space(kind, "nd", p), _geom(kind), ru.ogeom(kind, Q1D)
    n = nd.ndofs
    ctx = linalg.Context()
    mk = lambda v: po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[np.array([v]), np.array([0.6 * v])])  # noqa: E731
    c_m, c_s, c_k = mk(-w * w * 2.08), mk(w * 0.35), po.CoeffCtx()
    Ar_loc = ceed.curlcurlmass_operator(geom, nd, c_m.pack(), c_k.pack())
    Ai_loc = ceed.ndmass_operator(geom, nd, c_s.pack())
    L = lib.load()
    assert not Ar_loc.two_rhs() and not Ar_loc.supports_split() and not Ar_loc.streams()
    ess = nd.ess_dofs()
    Ar = linalg.ParOperator(ctx, Ar_loc, ess, linalg.DIAG_ONE)
    Ai = linalg.ParOperator(ctx, Ai_loc, ess, linalg.DIAG_ZERO)
    L.pa_op_complex_fused.restype = C.c_int
    assert L.pa_op_complex_fused(Ar_loc.handle, Ai_loc.handle) == 0
    xr, xi = ru.vector(n, 41), ru.vector(n, 42)
    yr, yi = linalg.complex_mult(ctx, Ar, Ai, _dev(xr), _dev(xi), _new(n), _new(n))
    oR = util.FastParOperatorOracle(nd, ogeom, "hdivmass", np.concatenate([c_m.pack(), c_k.pack()]), ess, Q1D, c_m, c_k)
    oI = util.FastParOperatorOracle(nd, ogeom, "hcurl", c_s.pack(), ess, Q1D, c_s, policy=po.DIAG_ZERO)
    ref_r, ref_i = oR.mult(xr) - oI.mult(xi), oR.mult(xi) + oI.mult(xr)
    assert _rel(yr.cpu().numpy(), ref_r) < RTOL and _rel(yi.cpu().numpy(), ref_i) < RTOL


def test_fused_step_is_not_available():
    """pa_op_prepare_fused_step reports "not available" at six points: the smoothers take their unfused path."""
    op = _nd_operator("ogrid15", 5, "hdivmass", "aniso")
    op.set_essential(tu.space("ogrid15", "nd", 5).ess_dofs())
    avail = C.c_int(-1)
    lib.check(lib.load().pa_op_prepare_fused_step(op.handle, C.byref(avail)))
    assert avail.value == 0


def test_order_six_is_still_refused():
    from palace_amd.fem.fespace import NDHexSpace

    mesh = ru.mesh("ogrid15")
    nd = NDHexSpace(mesh, 6)
    geom = ceed.GeomFactorData(mesh, 7)
    op = ceed.ndmass_operator(geom, nd, util.make_ctx("aniso", 2)[1])
    x = _dev(ru.vector(nd.ndofs, 1))
    with pytest.raises(lib.PalaceAmdError, match=r"no H\(curl\) hex kernel for order 6 with 7 points"):
        op.mult(x, _new(nd.ndofs))
