"""Column form of the streaming H(curl) hex kernel (four points per direction): an element extruded along its local zeta axis has
D_c(qx, qy, qz) = wz(qz) r_c(qx, qy), and a lane of the kernel owns one column (qx, qy), so batches of four such elements read one
number per component and lane (QData::d_col) instead of four.  Every D form against the C oracle, next to the same operator with the
form switched off (PALACE_AMD_STREAM_COLUMN=0) and to the one-shot kernel, the copies of the flag words the masked apply, the fused
smoother step and the complex apply read, and meshes on which some or all elements must keep the per-point data.

Bounds: the oracle at the suite's 1e-12 (test-libceed.cpp:262 criterion); on against off at 1e-13, the bound of the affine test --
the compact rows replace numbers that agree to PALACE_AMD_AFFINE_TOL = 1e-13 by their mean."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import HexMesh, ogrid_cylinder  # noqa: E402
from tests import util  # noqa: E402

RTOL = 1e-12
Q1D = 4
FORMS = ["curl_packed", "mass_packed", "km_packed12", "curl_metric", "km_metric"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _with(mesh, x=None, elem_nodes=None):
    """Copy of the mesh with other coordinates / connectivity and three attributes (the attribute -> material indirection)."""
    m = HexMesh(x=mesh.x.copy() if x is None else x, elem_nodes=mesh.elem_nodes if elem_nodes is None else elem_nodes,
                attr=(np.arange(mesh.ne) % 3 + 1).astype(np.int32))
    m.check()
    return m


def _base():
    # 160 elements: 0-31 the central block (affine), 32-159 the outer blocks (curved in the plane, extruded along local zeta)
    return ogrid_cylinder(4, 2)


CENTRAL = np.arange(160) < 32


def _expected(geom, sep, aff):
    """What stream_column() and stream_affine() must report when the caller's elements flagged in `sep` / `aff` are the
    column-separable / affine ones: a batch is four consecutive elements in the library's own element order; all-affine batches
    read the affine rows, the other batches of four separable elements the column rows."""
    ne = sep.size
    order = np.zeros(ne, dtype=np.int32)
    ceed._lib.check(ceed._lib.load().pa_geom_element_order(geom.handle, order.ctypes.data_as(ceed.C.c_void_p)))
    sep_b, aff_b = (sep | aff)[order].reshape(-1, 4).all(axis=1), aff[order].reshape(-1, 4).all(axis=1)
    n_aff_b = 4 * int(aff_b.sum())
    return ((ne, int((sep | aff).sum()), 4 * int((sep_b & ~aff_b).sum())),
            (ne, int(aff.sum()), n_aff_b))


def _build(mesh, nd, form):
    _, b_a = util.make_ctx("aniso", nattr=3)
    _, b_s = util.make_ctx("scalar", nattr=3)
    geom = ceed.GeomFactorData(mesh, Q1D)
    if form == "curl_packed":
        return geom, ceed.curlcurl_operator(geom, nd, b_a), "hdiv", b_a
    if form == "curl_metric":  # (the caller has set PALACE_AMD_DSTAGE=metric)
        return geom, ceed.curlcurl_operator(geom, nd, b_s), "hdiv", b_s
    if form == "mass_packed":
        return geom, ceed.ndmass_operator(geom, nd, b_a), "hcurl", b_a
    if form == "km_metric":
        return geom, ceed.curlcurlmass_operator(geom, nd, b_s, b_s), "hdivmass", np.concatenate([b_s, b_s])
    return geom, ceed.curlcurlmass_operator(geom, nd, b_a, b_a), "hdivmass", np.concatenate([b_a, b_a])


def _check(mesh, p, form, monkeypatch, sep, aff, seed=3):
    """The operator on `mesh` against the oracle (plain, one-shot, essential dofs fused) and against itself with the form off;
    sep / aff: the elements that are column-separable / affine by construction of the mesh.  Returns the two reports."""
    if form == "curl_metric":
        monkeypatch.setenv("PALACE_AMD_DSTAGE", "metric")
    nd = NDHexSpace(mesh, p)
    ogeom = util.oracle_geom(mesh, Q1D)
    x = np.random.default_rng(seed).uniform(-1, 1, nd.ndofs)
    xd = _dev(x)
    geom, op, qf, blob = _build(mesh, nd, form)
    assert op.streams()
    expect_col, expect_aff = _expected(geom, sep, aff)
    assert op.stream_column() == expect_col, (op.stream_column(), expect_col)
    assert op.stream_affine() == expect_aff, (op.stream_affine(), expect_aff)
    ref = util.oracle_apply_c(nd, ogeom, qf, blob, x, Q1D)
    y = op.mult(xd, torch.empty_like(xd)).cpu().numpy()
    print(f"{form} p={p}: vs oracle {_rel(y, ref):.2e}")
    assert _rel(y, ref) < RTOL
    y_one_shot = op.add_mult(xd, torch.zeros_like(xd)).cpu().numpy()
    assert _rel(y_one_shot, ref) < RTOL
    # masked apply (the _bc copy of the flag words) with the fix-up fused
    ess = nd.ess_dofs()
    K = linalg.ParOperator(linalg.Context(), op, ess, linalg.DIAG_ONE)
    yk = K.mult(xd, torch.empty_like(xd)).cpu().numpy()
    xm = x.copy()
    xm[ess] = 0.0
    refk = util.oracle_apply_c(nd, ogeom, qf, blob, xm, Q1D)
    refk[ess] = x[ess]
    assert _rel(yk, refk) < RTOL
    assert np.array_equal(yk[ess], x[ess])
    monkeypatch.setenv("PALACE_AMD_STREAM_COLUMN", "0")
    geom0, op0, _, _ = _build(mesh, nd, form)
    assert op0.stream_column() == (mesh.ne, 0, 0)
    assert op0.stream_affine() == expect_aff
    y0 = op0.mult(xd, torch.empty_like(xd)).cpu().numpy()
    print(f"{form} p={p}: on vs off {_rel(y, y0):.2e}")
    assert _rel(y0, ref) < RTOL and _rel(y, y0) < 1e-13
    if expect_col[2]:
        assert not np.array_equal(y, y0)  # (the compact rows were read: the two forms differ in the last bits)
    else:
        assert np.array_equal(y, y0)
    monkeypatch.delenv("PALACE_AMD_STREAM_COLUMN")
    return expect_col, expect_aff


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_every_form_on_the_extruded_mesh(monkeypatch, p, form):
    """Every element is column-separable; the outer blocks' batches take the column form, the central block's stay affine."""
    mesh = _with(_base())
    col, aff = _check(mesh, p, form, monkeypatch, sep=np.ones(160, bool), aff=CENTRAL)
    assert col[1] == 160 and aff[1] == 32 and col[2] + aff[2] == 160 and col[2] >= 128


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (2, "km_metric"), (1, "km_packed12")])
def test_mixed_batches_fall_back_to_per_point_data(monkeypatch, p, form):
    """The centre node (local lattice node 13: owned by one element) of one central-block and of one outer-block element moved by
    5 % of the element's size in x: exactly those two batches keep the per-point data."""
    base = _base()
    x = base.x.copy()
    for e in (5, 70):  # central block: elements 0-31, outer blocks: 32-159
        xe = base.x[base.elem_nodes[e], 0]
        x[base.elem_nodes[e, 13], 0] += 0.05 * (xe.max() - xe.min())
    mesh = _with(base, x=x)
    moved = np.isin(np.arange(160), (5, 70))
    col, aff = _check(mesh, p, form, monkeypatch, sep=~moved, aff=CENTRAL & ~moved)
    assert col[1] == 158 and aff[1] == 31 and col[2] + aff[2] == 160 - 8  # (the two elements sit in different batches)


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (3, "km_metric"), (2, "km_packed12"), (1, "curl_metric")])
def test_quadratic_layers_are_not_separable(monkeypatch, p, form):
    """Every mid-layer node plane shifted by 5 % of the layer height: z is quadratic in zeta, no element is separable (or affine)."""
    base = _base()
    zs = np.unique(np.round(base.x[:, 2], 9))
    assert zs.size == 5
    h = zs[2] - zs[0]
    x = base.x.copy()
    mid = np.isclose(x[:, 2], zs[1]) | np.isclose(x[:, 2], zs[3])
    x[mid, 2] += 0.05 * h
    mesh = _with(base, x=x)
    col, aff = _check(mesh, p, form, monkeypatch, sep=np.zeros(160, bool), aff=np.zeros(160, bool))
    assert col == (160, 0, 0) and aff == (160, 0, 0)


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (3, "km_metric"), (2, "mass_packed"), (1, "km_packed12")])
def test_graded_linear_layers_stay_separable(monkeypatch, p, form):
    """Unequal layers with the mid nodes exactly midway: z stays linear in zeta, every element separable."""
    base = _base()
    zs = np.unique(np.round(base.x[:, 2], 9))
    H = zs[-1]
    new = np.array([0.0, 0.15 * H, 0.3 * H, 0.65 * H, H])
    x = base.x.copy()
    x[:, 2] = np.interp(base.x[:, 2], zs, new)
    mesh = _with(base, x=x)
    col, aff = _check(mesh, p, form, monkeypatch, sep=np.ones(160, bool), aff=CENTRAL)
    assert col[1] == 160 and col[2] + aff[2] == 160


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (3, "km_metric"), (2, "curl_metric"), (1, "mass_packed")])
def test_extrusion_along_another_local_axis(monkeypatch, p, form):
    """A cyclic (orientation-preserving) permutation of the local axes of every element: the extrusion runs along local xi, where
    the kernel does not look for it.  No column batch; the affine block is unaffected (and separable by construction)."""
    base = _base()
    i, j, k = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    lat = np.empty(27, dtype=np.int64)
    lat[(i + 3 * j + 9 * k).ravel()] = (j + 3 * k + 9 * i).ravel()  # new (xi, eta, zeta) = old (zeta, xi, eta)
    mesh = _with(base, elem_nodes=base.elem_nodes[:, lat])
    J = mesh.jacobian_at(np.array([[0.3, 0.6, 0.2]]))[:, 0]
    assert np.all(np.abs(J[:, :2, 0]) < 1e-12) and np.all(np.abs(J[:, 2, 1:]) < 1e-12)  # z along xi only
    col, aff = _check(mesh, p, form, monkeypatch, sep=np.zeros(160, bool), aff=CENTRAL)
    assert col[1:] == (32, 0) and aff[1] == 32


class _Levels:
    """(K + M) at orders 1, 2, 3 on the extruded mesh with essential dofs, as the smoothers of the PCG loop see it."""

    def __init__(self, mesh):
        self.ctx = linalg.Context()
        self.geom = ceed.GeomFactorData(mesh, Q1D)
        _, bm = util.make_ctx("scalar")
        _, bc = util.make_ctx("identity")
        self.spaces = [NDHexSpace(mesh, p) for p in (1, 2, 3)]
        fine = ceed.curlcurlmass_operator(self.geom, self.spaces[-1], bm, bc)
        self.local = [fine.coarsen(self.geom, s) for s in self.spaces[:-1]] + [fine]
        self.A = [linalg.ParOperator(self.ctx, op, s.ess_dofs(), linalg.DIAG_ONE) for op, s in zip(self.local, self.spaces)]


@pytest.fixture(scope="module")
def levels_on_off():
    import os

    mesh = _base()
    out = {}
    prev = os.environ.get("PALACE_AMD_STREAM_COLUMN")
    try:
        for sw in ("1", "0"):
            os.environ["PALACE_AMD_STREAM_COLUMN"] = sw
            out[sw] = _Levels(mesh)
    finally:
        if prev is None:
            del os.environ["PALACE_AMD_STREAM_COLUMN"]
        else:
            os.environ["PALACE_AMD_STREAM_COLUMN"] = prev
    return out


@pytest.mark.parametrize("first_kind", [False, True])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_fused_chebyshev_step_and_residual(levels_on_off, level, first_kind):
    """The `_all` copy of the flag words: the smoother step and the residual evaluated in the epilogue of the E^T gather
    (zero and non-zero initial guess), column form on against off."""
    on, off = levels_on_off["1"], levels_on_off["0"]
    col, aff = on.local[level].stream_column(), on.local[level].stream_affine()
    assert col[:2] == (160, 160) and col[2] >= 128 and col[2] + aff[2] == 160 and off.local[level].stream_column() == (160, 0, 0)
    n = on.spaces[level].ndofs
    S = linalg.chebyshev(on.ctx, on.A[level], order=6, fourth_kind=not first_kind)
    S0 = linalg.chebyshev(off.ctx, off.A[level], order=6, fourth_kind=not first_kind)
    assert S.fused_step() and S0.fused_step()
    rng = np.random.default_rng(16)
    b = rng.uniform(-1, 1, n)
    b[on.spaces[level].ess_dofs()] = 0.0
    y = S.mult(_dev(b), _new(n)).cpu().numpy()
    y0 = S0.mult(_dev(b), _new(n)).cpu().numpy()
    g = rng.uniform(-1, 1, n)
    g[on.spaces[level].ess_dofs()] = 0.0
    z = S.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    z0 = S0.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    print(f"level {level}: step {_rel(y, y0):.2e}, with residual {_rel(z, z0):.2e}")
    assert _rel(y, y0) < 1e-13 and _rel(z, z0) < 1e-13


@pytest.mark.parametrize("p", [1, 2, 3])
def test_one_pass_complex_metric_apply(p):
    """The complex form of the metric kernel (two elements times two parts per batch) on column batches: y = (A_r + i A_i) x in one
    pass against its four real applies, plain and with essential dofs; 1e-13 of the largest entry, the bound the fused complex
    apply is held to against its separate applies elsewhere in the suite."""
    mesh = _base()
    mesh.attr[:] = 1 + (np.arange(mesh.ne) % 2)
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    two = lambda a, b: ceed.coefficient_context(3, attr_mat=[0, 1], mat_coeff=[np.asarray(a, float), np.asarray(b, float)])  # noqa: E731
    Ar = ceed.curlcurlmass_operator(geom, nd, two(-0.9, -0.35), two(1.0, 0.6))
    Ai = ceed.ndmass_operator(geom, nd, two(0.21, 0.05))
    assert ceed._lib.load().pa_op_complex_fused(Ar.handle, Ai.handle) == 1
    assert Ar.stream_column()[:2] == (160, 160) and Ar.stream_column()[2] + Ar.stream_affine()[2] == 160
    ctx = linalg.Context()
    n = nd.ndofs
    rng = np.random.default_rng(3)
    xr, xi = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    for ess in (np.zeros(0, np.int32), nd.ess_dofs()):
        A = linalg.ComplexParOperator(ctx, Ar, Ai, ess, linalg.DIAG_ONE)
        yr, yi = _new(n), _new(n)
        A.mult(_dev(xr), _dev(xi), yr, yi)
        tr, ti = xr.copy(), xi.copy()
        tr[ess] = 0.0
        ti[ess] = 0.0
        ap = lambda op, v: op.mult(_dev(v), _new(n)).cpu().numpy()  # noqa: E731
        er = ap(Ar, tr) - ap(Ai, ti)
        ei = ap(Ai, tr) + ap(Ar, ti)
        er[ess], ei[ess] = xr[ess], xi[ess]
        assert np.abs(yr.cpu().numpy() - er).max() < 1e-13 * np.abs(er).max()
        assert np.abs(yi.cpu().numpy() - ei).max() < 1e-13 * np.abs(ei).max()
