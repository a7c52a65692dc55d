"""The hexahedral kernels under rotated elements and fragmented dof numberings.

A. every kernel family against the C oracle on the reference's cylinder mesh with every element handed over in one of the 24
   rotations of the reference cube (tests/util.py: rotate_elements; every face class (ou, ov, swap) on every local face);
B. invariance on the device: rotating elements changes the element frames and nothing else, so skeleton rows (edge and face
   dofs) of the operators, the p-transfer and the gradient are the same numbers on both meshes, and the spectrum is the same
   (tests/test_orient_oracle.py states the same through the oracle alone);
C. the fused forms (essential rows, split vectors, smoother step, one-pass complex apply, affine batches) on rotated meshes;
D. the run-compressed index of the streaming kernels (pa_stream_host.hpp) at its capacity and just above it;
E. a numbering the index refuses: the operator keeps the one-shot kernel and every entry point stays correct.

Criteria: 1e-12 relative against the oracle (test/unit/test-libceed.cpp:245-282), 1e-13 between two device schedules of one
operator, bit equality where the same kernel computes the same sums, 1e-11 for curl grad = 0 (tests/test_hiptmair_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import H1HexSpace, NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import ogrid_cylinder  # noqa: E402
from tests import util  # noqa: E402
from tests.test_complex_gpu import _tensors  # noqa: E402
from tests.test_h1_gpu import _ctxs as _h1_ctxs, _oracle as _h1_oracle  # noqa: E402
from tests.test_split_gpu import _check_split  # noqa: E402

RTOL = 1e-12


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _nan(n):
    """an output vector that shows every entry the apply does not write"""
    return torch.full((n,), np.nan, dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _with_attr(mesh):
    """three attributes: the attribute -> material indirection of the per-element coefficients"""
    return type(mesh)(x=mesh.x, elem_nodes=mesh.elem_nodes, attr=(np.arange(mesh.ne) % 3 + 1).astype(np.int32),
                      bdr_faces=mesh.bdr_faces, bdr_attr=mesh.bdr_attr)


@pytest.fixture(scope="module")
def mesh80(cylinder_mesh):
    return _with_attr(cylinder_mesh)


@pytest.fixture(scope="module")
def mesh80_rot(mesh80):
    return util.rotate_elements(mesh80, util.seeded_rotations(mesh80.ne, 24))


@pytest.fixture(scope="module")
def mesh10():
    return _with_attr(ogrid_cylinder(1, 2))


_ogeom_cache = {}


def _ogeom(mesh, q1d):
    """the oracle's geometry factors, once per (mesh, rule)"""
    key = (id(mesh), q1d)
    if key not in _ogeom_cache:
        _ogeom_cache[key] = (mesh, util.oracle_geom(mesh, q1d))
    return _ogeom_cache[key][1]


def _nd_operator(geom, nd, qf, kind, dense=None):
    """(device operator, blob, oracle contexts) of K | M | K + M with material `kind` (K + M: both terms of that kind, the
    non-symmetric tensor next to a scalar mass)"""
    ck, bk = util.make_ctx(kind, nattr=3)
    cs, bs = util.make_ctx("scalar", nattr=3)
    if qf == "hdiv":
        return ceed.curlcurl_operator(geom, nd, bk, dense), bk, (ck, None)
    if qf == "hcurl":
        return ceed.ndmass_operator(geom, nd, bk, dense), bk, (ck, None)
    cm, bm = (cs, bs) if kind == "nonsym" else (ck, bk)
    return ceed.curlcurlmass_operator(geom, nd, bm, bk, dense), np.concatenate([bm, bk]), (cm, ck)


# ---- A. every kernel family on the rotated mesh ---------------------------------------------------------------------------

def test_rotated_geometry_factors(mesh80_rot):
    for q1d in (2, 3, 4, 5):
        g = ceed.GeomFactorData(mesh80_rot, q1d).to_numpy()
        ref = _ogeom(mesh80_rot, q1d)
        assert np.array_equal(g[:, 0, :], ref[:, 0, :])
        np.testing.assert_allclose(g[:, 1:, :], ref[:, 1:, :], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("p,q1d,form", [(1, 4, "stream"), (2, 4, "stream"), (3, 4, "stream"),
                                        (1, 5, "stream"), (2, 5, "stream"), (3, 5, "stream"), (4, 5, "stream"),
                                        (1, 3, "one-shot"), (2, 3, "one-shot"), (2, 4, "dense"), (2, 5, "dense")])
def test_rotated_nd_apply(mesh80_rot, p, q1d, form):
    """K, M, K + M with a scalar, a symmetric and a general tensor on the four-point streaming kernel, the five-point one (order 4
    and the coarsened levels of an order-4 problem, (2, 5) among them), the one-shot kernel and the dense-table form."""
    mesh = mesh80_rot
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, q1d)
    ogeom = _ogeom(mesh, q1d)
    dense = util.dense_tables(nd, q1d) if form == "dense" else None
    x = np.random.default_rng(100 * p + q1d).uniform(-1, 1, nd.ndofs)
    xd = _dev(x)
    worst = 0.0
    for kind in ("scalar", "aniso", "nonsym"):
        for qf in ("hdiv", "hcurl", "hdivmass"):
            op, blob, (c0, c1) = _nd_operator(geom, nd, qf, kind, dense)
            ref = util.oracle_apply_c(nd, ogeom, qf, blob, x, q1d)
            y = op.mult(xd, _nan(nd.ndofs)).cpu().numpy()
            worst = max(worst, _rel(y, ref))
            assert _rel(y, ref) < RTOL, (kind, qf, _rel(y, ref))
            if kind != "nonsym" and form != "dense":  # (a general tensor is applied matrix-free by the one-shot kernel)
                assert op.streams() == (form == "stream"), (kind, qf)
            if op.streams():
                assert np.array_equal(op.mult(xd, _new(nd.ndofs)).cpu().numpy(), y)  # fixed summation order
                y1 = op.add_mult(xd, torch.zeros_like(xd)).cpu().numpy()  # the one-shot kernel
                assert _rel(y1, ref) < RTOL, (kind, qf, "add_mult")
            if op.streams() and p <= 2:
                d = op.assemble_diagonal(_new(nd.ndofs)).cpu().numpy()
                dref = util.oracle_operator(nd, ogeom, qf, c0, c1, q1d).diagonal()
                assert _rel(d, dref) < RTOL, (kind, qf, "diagonal")
    print(f"rotated mesh, ND p = {p}, q1d = {q1d}, {form}: worst error against the oracle {worst:.2e}")


@pytest.mark.parametrize("p", [1, 2, 3])
def test_rotated_h1_apply(mesh80_rot, p):
    """H1 diffusion and diffusion + mass at four points per direction (order 3: the streaming kernel)."""
    mesh, q1d = mesh80_rot, 4
    h1 = H1HexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, q1d)
    ogeom = _ogeom(mesh, q1d)
    c_mass, c_diff = _h1_ctxs()
    x = np.random.default_rng(p).uniform(-1, 1, h1.ndofs)
    for qf in ("diffusion", "diffusionmass"):
        if qf == "diffusion":
            op, o = ceed.diffusion_operator(geom, h1, c_diff.pack()), _h1_oracle(h1, ogeom, po.QF_HCURL, c_diff, None, q1d)
        else:
            op, o = (ceed.diffusionmass_operator(geom, h1, c_mass.pack(), c_diff.pack()),
                     _h1_oracle(h1, ogeom, po.QF_HCURLMASS, c_mass, c_diff, q1d))
        assert op.streams() == (p == 3)
        ref = o.apply_add(x, np.zeros(h1.ndofs))
        y = op.mult(_dev(x), _new(h1.ndofs)).cpu().numpy()
        print(f"rotated mesh, H1 p = {p} {qf}: {_rel(y, ref):.2e}")
        assert _rel(y, ref) < RTOL
        assert np.array_equal(op.mult(_dev(x), _new(h1.ndofs)).cpu().numpy(), y)
        assert _rel(op.add_mult(_dev(x), torch.zeros(h1.ndofs, dtype=torch.float64, device="cuda")).cpu().numpy(), ref) < RTOL
        d = op.assemble_diagonal(_new(h1.ndofs)).cpu().numpy()
        assert _rel(d, o.diagonal()) < RTOL


# ---- B. invariance on the device ------------------------------------------------------------------------------------------

def _skeleton_error(ya, yb, n_skel):
    return np.abs(ya[:n_skel] - yb[:n_skel]).max() / np.abs(ya).max()


@pytest.mark.parametrize("p,q1d", [(3, 4), (4, 5)])
def test_skeleton_rows_of_curlcurlmass(mesh80, mesh80_rot, p, q1d):
    x = np.random.default_rng(p).uniform(-1, 1, NDHexSpace(mesh80, p).ndofs)
    ys = []
    for mesh in (mesh80, mesh80_rot):
        nd = NDHexSpace(mesh, p)
        x[nd.int_base:] = 0.0
        op, _, _ = _nd_operator(ceed.GeomFactorData(mesh, q1d), nd, "hdivmass", "aniso")
        assert op.streams()
        ys.append(op.mult(_dev(x), _new(nd.ndofs)).cpu().numpy())
    err = _skeleton_error(ys[0], ys[1], nd.int_base)
    ia, ib = (np.sort(np.abs(y[nd.int_base:]).reshape(mesh.ne, -1), axis=1) for y in ys)
    erri = np.abs(ia - ib).max() / np.abs(ys[0]).max()
    print(f"K + M p = {p}, q1d = {q1d}: skeleton rows {err:.2e}, interior |y| per element {erri:.2e} (oracle alone: 2e-15)")
    assert err < RTOL and erri < RTOL
    assert not np.array_equal(ys[0][nd.int_base:], ys[1][nd.int_base:])


def test_skeleton_rows_of_h1_streaming_kernel(mesh80, mesh80_rot):
    p, q1d = 3, 4
    c_mass, c_diff = _h1_ctxs()
    x = np.random.default_rng(8).uniform(-1, 1, H1HexSpace(mesh80, p).ndofs)
    for qf in ("diffusion", "diffusionmass"):
        ys = []
        for mesh in (mesh80, mesh80_rot):
            h1 = H1HexSpace(mesh, p)
            x[h1.int_base:] = 0.0
            geom = ceed.GeomFactorData(mesh, q1d)
            op = (ceed.diffusion_operator(geom, h1, c_diff.pack()) if qf == "diffusion" else
                  ceed.diffusionmass_operator(geom, h1, c_mass.pack(), c_diff.pack()))
            assert op.streams()
            ys.append(op.mult(_dev(x), _new(h1.ndofs)).cpu().numpy())
        err = _skeleton_error(ys[0], ys[1], h1.int_base)
        print(f"H1 p = 3 {qf}: skeleton rows {err:.2e}")
        assert err < RTOL


@pytest.mark.parametrize("pc,pf", [(2, 3), (2, 4)])
def test_skeleton_rows_of_p_transfer(mesh80, mesh80_rot, pc, pf):
    ctx = linalg.Context()
    rng = np.random.default_rng(pc + pf)
    nc, nf = NDHexSpace(mesh80, pc), NDHexSpace(mesh80, pf)
    xa, xb, xf = rng.uniform(-1, 1, nc.ndofs), rng.uniform(-1, 1, nc.ndofs), rng.uniform(-1, 1, nf.ndofs)
    xb[:nc.int_base] = xa[:nc.int_base]  # any interior entries: no tangential trace on the skeleton
    xf[nf.int_base:] = 0.0
    out = []
    for mesh, xc in ((mesh80, xa), (mesh80_rot, xb)):
        P = linalg.Interp(ctx, NDHexSpace(mesh, pc), NDHexSpace(mesh, pf))
        out.append((P.mult(_dev(xc), _new(nf.ndofs)).cpu().numpy(), P.mult_transpose(_dev(xf), _new(nc.ndofs)).cpu().numpy()))
    err = _skeleton_error(out[0][0], out[1][0], nf.int_base)
    errt = _skeleton_error(out[0][1], out[1][1], nc.int_base)
    print(f"P {pc} -> {pf}: skeleton rows {err:.2e}, of the transpose {errt:.2e} (oracle alone: 6e-16)")
    assert err < RTOL and errt < RTOL


@pytest.mark.parametrize("p", [2, 3])
def test_gradient_on_rotated_mesh(mesh80, mesh80_rot, p):
    ctx = linalg.Context()
    q1d = p + 1
    rng = np.random.default_rng(p)
    h0 = H1HexSpace(mesh80, p)
    phi0 = rng.uniform(-1, 1, h0.ndofs)
    phi0[h0.int_base:] = 0.0
    gs = []
    for mesh in (mesh80, mesh80_rot):
        h1, nd = H1HexSpace(mesh, p), NDHexSpace(mesh, p)
        G = linalg.Gradient(ctx, h1, nd)
        gs.append(G.mult(_dev(phi0), _new(nd.ndofs)).cpu().numpy())
    err = _skeleton_error(gs[0], gs[1], nd.int_base)
    # on the rotated mesh (h1, nd, G of the last pass): curl grad = 0 and G^T M G = A_H1, any phi
    phi = rng.uniform(-1, 1, h1.ndofs)
    g = G.mult(_dev(phi), _new(nd.ndofs))
    geom = ceed.GeomFactorData(mesh80_rot, q1d)
    eps = ceed.coefficient_context(3, attr_mat=[0, 0, 0], mat_coeff=[np.array([2.08])])
    K = ceed.curlcurl_operator(geom, nd, ceed.coefficient_context(3))
    M = ceed.ndmass_operator(geom, nd, eps)
    A = ceed.diffusion_operator(geom, h1, eps)
    kg = K.mult(g, _new(nd.ndofs)).cpu().numpy()
    mg = M.mult(g, _new(nd.ndofs))
    ratio = np.abs(kg).max() / np.abs(mg.cpu().numpy()).max()
    gtmg = G.mult_transpose(mg, _new(h1.ndofs)).cpu().numpy()
    aphi = A.mult(_dev(phi), _new(h1.ndofs)).cpu().numpy()
    print(f"G p = {p}: skeleton rows {err:.2e}, |K G phi| / |M G phi| = {ratio:.2e} (oracle alone: 1.4e-14), "
          f"G^T M G against A_H1 {_rel(gtmg, aphi):.2e}")
    assert err < RTOL
    assert ratio < 1e-11
    assert np.linalg.norm(gtmg - aphi) < 1e-11 * np.linalg.norm(aphi)


def test_spectrum_on_rotated_mesh(mesh10):
    """K + M at order 2 on ten elements (320 dofs), assembled from applies to unit vectors on the four-point streaming kernel."""
    p, q1d = 2, 4
    rot = util.rotate_elements(mesh10, util.seeded_rotations(mesh10.ne, 3))
    lam = []
    for mesh in (mesh10, rot):
        nd = NDHexSpace(mesh, p)
        assert nd.ndofs == 320
        op, _, _ = _nd_operator(ceed.GeomFactorData(mesh, q1d), nd, "hdivmass", "aniso")
        assert op.streams()
        eye = torch.eye(nd.ndofs, dtype=torch.float64, device="cuda")
        cols = torch.empty_like(eye)
        for j in range(nd.ndofs):
            op.mult(eye[j], cols[j])
        A = cols.cpu().numpy().T
        assert np.abs(A - A.T).max() < 1e-13 * np.abs(A).max()
        lam.append(np.linalg.eigvalsh(0.5 * (A + A.T)))
    err = np.abs(lam[0] - lam[1]).max() / lam[0][-1]
    print(f"spectrum of K + M, 320 dofs: {err:.2e} of lambda_max = {lam[0][-1]:.4g} (oracle alone: 2.3e-15)")
    assert lam[0][0] > 0.0 and err < RTOL


# ---- C. fused forms on the rotated mesh -----------------------------------------------------------------------------------

def _par_operator_check(nd, ogeom, q1d, local, blob, ctxs):
    """ParOperator::Mult (rap.cpp:195-234) with both diagonal policies against the oracle, essential rows bit for bit"""
    ess = nd.ess_dofs()
    assert ess.size > 0
    lctx = linalg.Context()
    x = np.random.default_rng(5).uniform(-1, 1, nd.ndofs)
    for policy, opol in ((linalg.DIAG_ONE, po.DIAG_ONE), (linalg.DIAG_ZERO, po.DIAG_ZERO)):
        A = linalg.ParOperator(lctx, local, ess, policy)
        y = A.mult(_dev(x), _nan(nd.ndofs)).cpu().numpy()
        ref = util.FastParOperatorOracle(nd, ogeom, "hdivmass", blob, ess, q1d, ctxs[0], ctxs[1], policy=opol).mult(x)
        assert _rel(y, ref) < RTOL, (policy, _rel(y, ref))
        assert np.array_equal(y[ess], x[ess] if policy == linalg.DIAG_ONE else np.zeros(ess.size))


def _chebyshev_check(monkeypatch, A, ess, n, expect_fused):
    """the smoother with its step in the E^T epilogue against the same smoother with the step as a vector kernel"""
    lctx = A.ctx
    S = linalg.chebyshev(lctx, A, order=4)
    if expect_fused is not None:
        assert S.fused_step() == expect_fused
    monkeypatch.setenv("PALACE_AMD_FUSED_STEP", "0")
    S0 = linalg.chebyshev(lctx, A, order=4)
    monkeypatch.delenv("PALACE_AMD_FUSED_STEP")
    assert not S0.fused_step() and S0.lambda_max() == S.lambda_max()
    rng = np.random.default_rng(21)
    b, g = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b[ess] = 0.0
    g[ess] = 0.0
    y = S.mult(_dev(b), _new(n)).cpu().numpy()
    y0 = S0.mult(_dev(b), _new(n)).cpu().numpy()
    z = S.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    z0 = S0.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    assert np.isfinite(y0).all() and np.abs(y0).max() > 0.0
    assert _rel(y, y0) < 1e-13 and _rel(z, z0) < 1e-13, (_rel(y, y0), _rel(z, z0))


def _complex_operators(geom, nd):
    """real part: tensor mass + tensor curl-curl, imaginary part: tensor mass
    (tests/test_stream5_aniso_gpu.py: test_fused_complex_apply_aniso_five_points_with_surface_terms without the surface terms)"""
    T = _tensors()
    two = lambda a, b: ceed.coefficient_context(3, attr_mat=[0, 1, 0], mat_coeff=[np.asarray(a, float), np.asarray(b, float)])  # noqa: E731
    Ar = ceed.curlcurlmass_operator(geom, nd, two(T["mr0"], T["mr1"]), two(T["cr0"], T["cr1"]))
    Ai = ceed.ndmass_operator(geom, nd, two(T["mi0"], T["mi1"]))
    return Ar, Ai


def _complex_check(Ar, Ai, ess, n, build_parts):
    """ComplexParOperator::Mult against the four real applies (linalg/operator.cpp:98-134) of separately built operators"""
    lctx = linalg.Context()
    Br, Bi = build_parts()
    rng = np.random.default_rng(8)
    xr, xi = (_dev(rng.uniform(-1, 1, n)) for _ in range(2))

    def app(o, v):
        return o.mult(v, torch.empty_like(v))

    for e in (np.zeros(0, np.int32), ess):
        A = linalg.ComplexParOperator(lctx, Ar, Ai, e, linalg.DIAG_ONE)
        yr, yi = _new(n), _new(n)
        A.mult(xr, xi, yr, yi)
        mr, mi = xr.clone(), xi.clone()
        ed = torch.from_numpy(e.astype(np.int64)).cuda()
        mr[ed], mi[ed] = 0.0, 0.0
        wr, wi = app(Br, mr) - app(Bi, mi), app(Bi, mr) + app(Br, mi)
        wr[ed], wi[ed] = xr[ed], xi[ed]
        scale = float(torch.maximum(wr.abs().max(), wi.abs().max()))
        er, ei = float((yr - wr).abs().max()) / scale, float((yi - wi).abs().max()) / scale
        assert er < 1e-13 and ei < 1e-13, (e.size, er, ei)


@pytest.mark.parametrize("p,q1d", [(2, 4), (4, 5)])
def test_rotated_fused_forms(mesh80_rot, monkeypatch, p, q1d):
    mesh = mesh80_rot
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, q1d)
    ogeom = _ogeom(mesh, q1d)
    local, blob, ctxs = _nd_operator(geom, nd, "hdivmass", "aniso")
    assert local.streams()
    _par_operator_check(nd, ogeom, q1d, local, blob, ctxs)
    make = lambda: _nd_operator(geom, nd, "hdivmass", "aniso")[0]  # noqa: E731
    _check_split(make, nd.ndofs, 30 + p)
    ess = nd.ess_dofs()
    A = linalg.ParOperator(linalg.Context(), make(), ess, linalg.DIAG_ONE)
    _chebyshev_check(monkeypatch, A, ess, nd.ndofs, True)
    Ar, Ai = _complex_operators(geom, nd)
    assert ceed._lib.load().pa_op_complex_fused(Ar.handle, Ai.handle) != 0
    _complex_check(Ar, Ai, ess, nd.ndofs, lambda: _complex_operators(geom, nd))


def test_rotated_affine_batches():
    """The central block of the O-grid (a fifth of the elements) has constant Jacobians, rotated or not: the same elements are
    found affine, and the compact D of their batches gives the oracle's result."""
    plain = _with_attr(ogrid_cylinder(4, 5))
    rot = util.rotate_elements(plain, util.seeded_rotations(plain.ne, 7))
    p, q1d = 3, 4
    counts = []
    for mesh in (plain, rot):
        nd = NDHexSpace(mesh, p)
        op, blob, _ = _nd_operator(ceed.GeomFactorData(mesh, q1d), nd, "hdivmass", "aniso")
        assert op.streams()
        counts.append(op.stream_affine())
    ne, n_aff, n_comp = counts[1]
    assert counts[0] == counts[1] and ne == rot.ne and n_aff == rot.ne // 5 and 0 < n_comp <= n_aff, counts
    x = np.random.default_rng(3).uniform(-1, 1, nd.ndofs)
    ref = util.oracle_apply_c(nd, util.oracle_geom(rot, q1d), "hdivmass", blob, x, q1d)
    y = op.mult(_dev(x), _new(nd.ndofs)).cpu().numpy()
    print(f"rotated O-grid, {n_comp} of {ne} elements on the compact D: {_rel(y, ref):.2e}")
    assert _rel(y, ref) < RTOL


# ---- D, E. fragmented and refused numberings --------------------------------------------------------------------------------

class _Case:
    """one space on the 80-element mesh in its natural numbering with its operator, input, result and oracle"""

    def __init__(self, mesh, kind, p, q1d):
        self.mesh, self.kind, self.p, self.q1d = mesh, kind, p, q1d
        self.space = (NDHexSpace if kind == "nd" else H1HexSpace)(mesh, p)
        self.geom = ceed.GeomFactorData(mesh, q1d)
        self.ogeom = _ogeom(mesh, q1d)
        self.n = self.space.ndofs
        self.x = np.random.default_rng(40 + p).uniform(-1, 1, self.n)
        self.op = self.build(self.space)
        self.y = self.op.mult(_dev(self.x), _new(self.n)).cpu().numpy()
        self.y_one_shot = self.op.add_mult(_dev(self.x), torch.zeros(self.n, dtype=torch.float64, device="cuda")).cpu().numpy()

    def build(self, space):
        if self.kind == "nd":
            return _nd_operator(self.geom, space, "hdivmass", "aniso")[0]
        return ceed.diffusion_operator(self.geom, space, _h1_ctxs()[1].pack())

    def oracle(self, space):
        """(apply, diagonal) of the oracle on `space`"""
        if self.kind == "nd":
            _, blob, (cm, cc) = _nd_operator(self.geom, space, "hdivmass", "aniso")
            return (lambda v: util.oracle_apply_c(space, self.ogeom, "hdivmass", blob, v, self.q1d),
                    lambda: util.oracle_operator(space, self.ogeom, "hdivmass", cm, cc, self.q1d).diagonal())
        o = _h1_oracle(space, self.ogeom, po.QF_HCURL, _h1_ctxs()[1], None, self.q1d)
        return (lambda v: o.apply_add(v, np.zeros(self.n))), o.diagonal


_cases = {}


def _case(mesh, kind, p, q1d):
    key = (id(mesh), kind, p, q1d)
    if key not in _cases:
        _cases[key] = _Case(mesh, kind, p, q1d)
    return _cases[key]


# (space, p, q1d, capacity of that kernel's index: kIdxMaxRuns, kWideMaxRuns, kIdxWords - kIdxStart0H1 of pa_stream_host.hpp)
CAPACITY_CASES = [("nd", 2, 4, 20), ("nd", 3, 4, 20), ("nd", 4, 5, 24), ("h1", 3, 4, 28)]


@pytest.mark.parametrize("kind,p,q1d,cap", CAPACITY_CASES)
@pytest.mark.parametrize("where,over", [("interior", 0), ("interior", 2), ("faces", 0)])
def test_index_at_and_above_its_capacity(mesh80, kind, p, q1d, cap, where, over):
    """Single dofs exchanged between far blocks of the natural numbering until an element has exactly `cap` runs (the streaming
    kernel decodes a full index block) or cap + 2 (build_stream keeps the one-shot kernel): the same operator under another
    naming of its dofs."""
    c = _case(mesh80, kind, p, q1d)
    assert c.op.streams()
    perm, runs = util.fragmenting_permutation(c.space, where, cap + over)
    assert runs.max() == cap + over and util.element_runs(c.space.elem_dof_lex).max() < cap
    space = util.renumbered(c.space, perm)
    op = c.build(space)
    assert op.streams() == (over == 0), (runs.max(), cap)
    xp = np.empty(c.n)
    xp[perm] = c.x
    yp = op.mult(_dev(xp), _new(c.n)).cpu().numpy()
    y = yp[perm]  # back in the natural numbering
    ref = c.oracle(space)[0](xp)
    print(f"{kind} p = {p}: {runs.max()} runs (capacity {cap}), streams = {op.streams()}, against the natural numbering "
          f"{_relmax(y, c.y):.2e}, against the oracle {_rel(yp, ref):.2e}")
    assert _rel(yp, ref) < RTOL
    if over == 0:
        assert np.array_equal(y, c.y)  # the same kernel, the same sums
    else:
        assert _relmax(y, c.y) < 1e-13  # another schedule
        assert np.array_equal(y, c.y_one_shot)  # ... the one AddMult takes on the natural numbering
    # essential rows through the same index
    ess = space.ess_dofs()
    A = linalg.ParOperator(linalg.Context(), op, ess, linalg.DIAG_ONE)
    ya = A.mult(_dev(xp), _new(c.n)).cpu().numpy()
    tx = xp.copy()
    tx[ess] = 0.0
    refa = c.oracle(space)[0](tx)
    refa[ess] = xp[ess]
    assert _rel(ya, refa) < RTOL and np.array_equal(ya[ess], xp[ess])


@pytest.mark.parametrize("kind,p,q1d", [("nd", 2, 4), ("nd", 4, 5), ("h1", 3, 4)])
def test_refused_numbering_is_still_a_correct_operator(mesh80, mesh10, monkeypatch, kind, p, q1d):
    """A random permutation of the dofs: every entry of an element is a run of its own, pack_index refuses, and every entry point
    either answers "no" or stays correct on the one-shot kernel."""
    c = _case(mesh80, kind, p, q1d)
    perm = np.random.default_rng(5).permutation(c.n)
    space = util.renumbered(c.space, perm)
    P = space.elem_dof_lex.shape[1]
    assert util.element_runs(space.elem_dof_lex).min() > P // 2  # (nearly one run per entry)
    op = c.build(space)
    assert not op.streams()
    apply_ref, diag_ref = c.oracle(space)
    n = c.n
    xp = np.empty(n)
    xp[perm] = c.x
    ref = apply_ref(xp)
    y = op.mult(_dev(xp), _new(n)).cpu().numpy()
    print(f"{kind} p = {p}, refused numbering: against the oracle {_rel(y, ref):.2e}, against the natural numbering "
          f"{_relmax(y[perm], c.y):.2e}")
    assert _rel(y, ref) < RTOL and _relmax(y[perm], c.y) < 1e-13
    y0 = np.random.default_rng(7).uniform(-1, 1, n)
    assert _rel(op.add_mult(_dev(xp), _dev(y0.copy())).cpu().numpy(), y0 + ref) < RTOL
    assert _rel(op.mult_transpose(_dev(xp), _new(n)).cpu().numpy(), ref) < RTOL  # (symmetric coefficients)
    x1 = np.random.default_rng(9).uniform(-1, 1, n)
    ya, yb = op.mult2(_dev(xp), _dev(x1), _new(n), _new(n))
    assert _rel(ya.cpu().numpy(), ref) < RTOL and _rel(yb.cpu().numpy(), apply_ref(x1)) < RTOL
    d = op.assemble_diagonal(_new(n)).cpu().numpy()
    dn = c.op.assemble_diagonal(_new(n)).cpu().numpy()
    assert _relmax(d[perm], dn) < 1e-13
    if p < 4:
        assert _rel(d, diag_ref()) < RTOL
    else:  # (the oracle's element matrices of order 4 take 0.1 s per element: the ten-element mesh, numbered at random as well)
        c10 = _case(mesh10, kind, p, q1d)
        s10 = util.renumbered(c10.space, np.random.default_rng(6).permutation(c10.n))
        op10 = c10.build(s10)
        assert not op10.streams()
        assert _rel(op10.assemble_diagonal(_new(c10.n)).cpu().numpy(), c10.oracle(s10)[1]()) < RTOL
    # ParOperator with the permuted essential list
    ess = space.ess_dofs()
    assert np.array_equal(ess, np.sort(perm[c.space.ess_dofs()]))
    for policy in (linalg.DIAG_ONE, linalg.DIAG_ZERO):
        A = linalg.ParOperator(linalg.Context(), c.build(space), ess, policy)
        ya = A.mult(_dev(xp), _new(n)).cpu().numpy()
        tx = xp.copy()
        tx[ess] = 0.0
        refa = apply_ref(tx)
        refa[ess] = xp[ess] if policy == linalg.DIAG_ONE else 0.0
        assert _rel(ya, refa) < RTOL and np.array_equal(ya[ess], refa[ess]), policy
    # split vectors: "no", or correct
    if op.supports_split():
        _check_split(lambda: c.build(space), n, 50 + p)
    # the smoother: built, and the same with or without the fused step
    A = linalg.ParOperator(linalg.Context(), c.build(space), ess, linalg.DIAG_ONE)
    _chebyshev_check(monkeypatch, A, ess, n, None)
    # one-pass complex apply: whatever pa_op_complex_fused says
    if kind == "nd":
        parts = lambda: _complex_operators(c.geom, space)  # noqa: E731
    else:
        c_mass, c_diff = _h1_ctxs()
        parts = lambda: (ceed.diffusion_operator(c.geom, space, c_diff.pack()),  # noqa: E731
                         ceed.diffusionmass_operator(c.geom, space, c_mass.pack(), c_diff.pack()))
    Ar, Ai = parts()
    print("    pa_op_complex_fused:", ceed._lib.load().pa_op_complex_fused(Ar.handle, Ai.handle), "supports_split:", op.supports_split())
    _complex_check(Ar, Ai, ess, n, parts)
