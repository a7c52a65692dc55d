"""Anisotropic (symmetric tensor) materials on the five-point streaming kernel (pa_nd_hex_stream5.hip): the real curl-curl + mass
operator on packed D -- twelve doubles per point, arriving as a mass and a curl-curl block -- with its split-vector form and the
smoother step fused into its gather, and the one-pass complex apply on the packed D of two such operators, at order 4 and on the
p-coarsened levels of an order-4 problem (p = 1, 2, 3 on the five-point rule).

Criteria: 1e-12 relative against the oracle (test/unit/test-libceed.cpp:245-282, as tests/test_stream5_gpu.py and
tests/test_complex_gpu.py), 1e-13 between two device schedules of the same operator, bit equality where the neighbouring tests
demand it (repeated applies, essential rows, split vectors)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import ogrid_cylinder, refine_uniform  # noqa: E402
from oracle import palace_oracle as po  # noqa: E402
from tests import util  # noqa: E402
from tests.test_complex_gpu import FUSED_CHECK, _tensors  # noqa: E402
from tests.test_split_gpu import _check_split  # noqa: E402

RTOL = 1e-12
Q1D = 5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _streams(op):
    return bool(ceed._lib.load().pa_op_streams(op.handle))


def _blobs(kinds):
    """(mass, curl-curl) coefficient contexts and blobs for a pair of kinds"""
    cm, bm = util.make_ctx(kinds[0], nattr=3)
    cc, bc = util.make_ctx(kinds[1], nattr=3)
    return cm, bm, cc, bc


@pytest.fixture(scope="module")
def mesh640(cylinder_mesh):
    m = refine_uniform(cylinder_mesh)
    # three attributes: the attribute -> material indirection of the per-element coefficients
    return type(m)(x=m.x, elem_nodes=m.elem_nodes, attr=(np.arange(m.ne) % 3 + 1).astype(np.int32))


@pytest.mark.parametrize("p,kinds", [(p, ("aniso", "aniso")) for p in (1, 2, 3, 4)] + [(4, ("scalar", "aniso")), (4, ("aniso", "scalar"))])
@pytest.mark.parametrize("wgx", [None, "1"])
def test_aniso_curlcurlmass_streams_and_matches_oracle(mesh640, monkeypatch, p, kinds, wgx):
    """K + M with tensor coefficients (one of them at least): the packed-D instantiation of the streaming kernel is selected and
    computes what the oracle and the one-shot kernel compute; with one workgroup per XCD every wave walks ~20 batches."""
    if wgx:
        monkeypatch.setenv("PALACE_AMD_STREAM_WGX", wgx)
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    _, bm, _, bc = _blobs(kinds)
    op = ceed.curlcurlmass_operator(geom, nd, bm, bc)
    assert _streams(op), "the streaming kernel was not selected"
    x = np.random.default_rng(3).uniform(-1, 1, nd.ndofs)
    y = op.mult(_dev(x), torch.full((nd.ndofs,), np.nan, dtype=torch.float64, device="cuda")).cpu().numpy()
    ref = util.oracle_apply_c(nd, util.oracle_geom(mesh, Q1D), "hdivmass", np.concatenate([bm, bc]), x, Q1D)
    print("stream vs oracle", p, kinds, wgx, _rel(y, ref))
    assert _rel(y, ref) < RTOL
    # bit-reproducible (fixed summation order of the run gather)
    y2 = op.mult(_dev(x), torch.empty(nd.ndofs, dtype=torch.float64, device="cuda")).cpu().numpy()
    assert np.array_equal(y, y2)
    # AddMult keeps the one-shot kernel: same operator, different schedule
    y3 = op.add_mult(_dev(x), _dev(ref.copy())).cpu().numpy()
    assert _rel(y3, 2 * ref) < RTOL
    # the one-shot form of the same operator (PALACE_AMD_STREAM5=0 at creation)
    monkeypatch.setenv("PALACE_AMD_STREAM5", "0")
    op1 = ceed.curlcurlmass_operator(geom, nd, bm, bc)
    assert not _streams(op1)
    y1 = op1.mult(_dev(x), torch.empty(nd.ndofs, dtype=torch.float64, device="cuda")).cpu().numpy()
    print("stream vs one-shot", p, kinds, wgx, _rel(y, y1))
    assert _rel(y, y1) < 1e-13


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("policy", ["one", "zero"])
def test_aniso_par_operator_essential_rows(mesh640, monkeypatch, p, policy):
    """ParOperator::Mult (rap.cpp:195-234) over the anisotropic K + M: essential dofs read as zero inside the kernel, their rows
    written by the run gather (x or 0), bit-exactly."""
    monkeypatch.setenv("PALACE_AMD_STREAM_WGX", "2")
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    cm, bm, cc, bc = _blobs(("aniso", "aniso"))
    local = ceed.curlcurlmass_operator(geom, nd, bm, bc)
    ess = nd.ess_dofs()
    ctx = linalg.Context()
    pol = linalg.DIAG_ONE if policy == "one" else linalg.DIAG_ZERO
    A = linalg.ParOperator(ctx, local, ess, pol)
    x = np.random.default_rng(5).uniform(-1, 1, nd.ndofs)
    y = A.mult(_dev(x), torch.full((nd.ndofs,), np.nan, dtype=torch.float64, device="cuda")).cpu().numpy()
    oracle = util.FastParOperatorOracle(nd, util.oracle_geom(mesh, Q1D), "hdivmass", np.concatenate([bm, bc]), ess, Q1D, cm, cc,
                                        policy=po.DIAG_ONE if policy == "one" else po.DIAG_ZERO)
    ref = oracle.mult(x)
    print("ParOperator vs oracle", p, policy, _rel(y, ref))
    assert _rel(y, ref) < RTOL
    assert np.array_equal(y[ess], x[ess] if policy == "one" else np.zeros(ess.size))


@pytest.mark.parametrize("p", [2, 4])
def test_aniso_split_vectors(mesh640, p):
    """The split-vector form (multi-rank applies without L-vector copies) of the packed-D K + M instantiation: bit-exact
    against the plain apply, essential rows included."""
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    _, bm, _, bc = _blobs(("aniso", "aniso"))
    make = lambda: ceed.curlcurlmass_operator(geom, nd, bm, bc)  # noqa: E731
    assert make().supports_split()
    _check_split(make, nd.ndofs, 30 + p)


@pytest.mark.parametrize("p", [2, 4])
def test_aniso_chebyshev_steps_fused_into_the_gather(mesh640, monkeypatch, p):
    """The smoother step evaluated in the E^T epilogue (pa_op_mult_cheb_step) on the anisotropic level operator: against the same
    smoother with the step as a vector kernel (PALACE_AMD_FUSED_STEP=0), zero and non-zero initial guess."""
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    _, bm, _, bc = _blobs(("aniso", "aniso"))
    local = ceed.curlcurlmass_operator(geom, nd, bm, bc)
    ess = nd.ess_dofs()
    ctx = linalg.Context()
    A = linalg.ParOperator(ctx, local, ess, linalg.DIAG_ONE)
    S = linalg.chebyshev(ctx, A, order=4)
    assert S.fused_step()
    monkeypatch.setenv("PALACE_AMD_FUSED_STEP", "0")
    S0 = linalg.chebyshev(ctx, A, order=4)
    assert not S0.fused_step() and S0.lambda_max() == S.lambda_max()
    n = nd.ndofs
    rng = np.random.default_rng(21)
    b, g = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b[ess] = 0.0
    g[ess] = 0.0
    y = S.mult(_dev(b), torch.empty(n, dtype=torch.float64, device="cuda")).cpu().numpy()
    y0 = S0.mult(_dev(b), torch.empty(n, dtype=torch.float64, device="cuda")).cpu().numpy()
    z = S.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    z0 = S0.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    print("fused step vs vector kernel", p, _rel(y, y0), _rel(z, z0))
    assert _rel(y, y0) < 1e-13 and _rel(z, z0) < 1e-13


def test_aniso_ragged_and_tiny_meshes():
    """Odd element counts (the last batch holds one element and one pad), fewer batches than XCDs."""
    for n, nz in ((1, 3), (1, 1)):
        mesh = ogrid_cylinder(n, nz)
        nd = NDHexSpace(mesh, 4)
        geom = ceed.GeomFactorData(mesh, Q1D)
        _, bm = util.make_ctx("aniso", nattr=int(mesh.attr.max()))
        _, bc = util.make_ctx("aniso", nattr=int(mesh.attr.max()))
        op = ceed.curlcurlmass_operator(geom, nd, bm, bc)
        assert _streams(op)
        x = np.random.default_rng(7).uniform(-1, 1, nd.ndofs)
        y = op.mult(_dev(x), torch.full((nd.ndofs,), np.nan, dtype=torch.float64, device="cuda")).cpu().numpy()
        ref = util.oracle_apply_c(nd, util.oracle_geom(mesh, Q1D), "hdivmass", np.concatenate([bm, bc]), x, Q1D)
        print("ragged", n, nz, mesh.ne, _rel(y, ref))
        assert _rel(y, ref) < RTOL, (n, nz, mesh.ne)


@pytest.mark.parametrize("p,mat", [(p, m) for p in (1, 2, 3, 4) for m in ("aniso", "aniso2")] + [(4, "aniso-odd"), (2, "aniso2-odd")])
def test_fused_complex_apply_aniso_five_points(p, mat, tmp_path):
    """y = (A_r + i A_i) x in one pass on the packed D of both operators (real part: tensor mass + tensor curl-curl; imaginary part:
    tensor mass, "aniso", or mass + curl-curl, "aniso2") at five points per direction: against the four separate applies
    (PALACE_AMD_COMPLEX_FUSED=0, linalg/operator.cpp:98-134) and against the oracle's operators combined as
    tests/test_complex_gpu.py: test_fused_complex_apply combines them; "-odd": 15 elements."""
    shape = (1, 3) if mat.endswith("-odd") else (2, 3)
    mat = mat.replace("-odd", "")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    tf = str(tmp_path / "tensors.npz")
    np.savez(tf, **_tensors())
    for fused in (1, 0):
        f = str(tmp_path / f"out{fused}.npz")
        r = subprocess.run([sys.executable, "-c", FUSED_CHECK % root, str(p), f, str(Q1D), mat, tf, str(shape[0]), str(shape[1])],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, PALACE_AMD_COMPLEX_FUSED=str(fused)))
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
        res[fused] = np.load(f)
    assert int(res[1]["fused"]) == 1 and int(res[0]["fused"]) == 0
    for k in ("plain_r", "plain_i", "ess_r", "ess_i", "plain_local_r", "plain_local_i"):
        a, b = res[1][k], res[0][k]
        print("one pass vs four applies", p, mat, k, np.abs(a - b).max() / np.abs(b).max())
        assert np.abs(a - b).max() < 1e-13 * np.abs(b).max(), k
    # oracle
    mesh = ogrid_cylinder(*shape)
    assert mesh.ne % 2 == (1 if shape == (1, 3) else 0)
    mesh.attr[:] = 1 + (np.arange(mesh.ne) % 2)
    nd = NDHexSpace(mesh, p)
    ogeom = util.oracle_geom(mesh, Q1D)
    off, ori = nd.native_restriction()
    interp, curl = util.dense_tables(nd, Q1D)
    two = lambda a, b: po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[np.asarray(a, float), np.asarray(b, float)])  # noqa: E731
    T = _tensors()
    Aro = po.CeedOperatorOracle(nd.ndofs, off, ori, interp, curl, ogeom, po.QF_HDIVMASS, two(T["mr0"], T["mr1"]), two(T["cr0"], T["cr1"]))
    Aio = (po.CeedOperatorOracle(nd.ndofs, off, ori, interp, curl, ogeom, po.QF_HCURL, two(T["mi0"], T["mi1"])) if mat == "aniso" else
           po.CeedOperatorOracle(nd.ndofs, off, ori, interp, curl, ogeom, po.QF_HDIVMASS, two(T["mi0"], T["mi1"]), two(T["ci0"], T["ci1"])))
    xr, xi = res[1]["xr"], res[1]["xi"]
    z = lambda: np.zeros(nd.ndofs)  # noqa: E731
    yr = Aro.apply_add(xr, z()) - Aio.apply_add(xi, z())
    yi = Aio.apply_add(xr, z()) + Aro.apply_add(xi, z())
    print("one pass vs oracle", p, mat, np.abs(res[1]["plain_r"] - yr).max() / np.abs(yr).max(),
          np.abs(res[1]["plain_i"] - yi).max() / np.abs(yi).max())
    assert np.abs(res[1]["plain_r"] - yr).max() < 1e-12 * np.abs(yr).max()
    assert np.abs(res[1]["plain_i"] - yi).max() < 1e-12 * np.abs(yi).max()
    ess = nd.ess_dofs()
    txr, txi = xr.copy(), xi.copy()
    txr[ess] = 0.0
    txi[ess] = 0.0
    er = Aro.apply_add(txr, z()) - Aio.apply_add(txi, z())
    ei = Aio.apply_add(txr, z()) + Aro.apply_add(txi, z())
    er[ess], ei[ess] = xr[ess], xi[ess]
    assert np.abs(res[1]["ess_r"] - er).max() < 1e-12 * np.abs(er).max()
    assert np.abs(res[1]["ess_i"] - ei).max() < 1e-12 * np.abs(ei).max()


def test_fused_complex_apply_aniso_five_points_with_surface_terms():
    """Order 4 with surface terms (tests/test_complex_gpu.py: test_fused_complex_apply_with_surface_terms[hex-aniso] carried to
    the five-point rule): the volume operators pair up in the one-pass kernel on packed D (pa_op_complex_fused = 3), the dense
    boundary sub-operators are applied after it to both parts of x.  Against the same operators applied one by one and combined
    term by term, plain and with essential dofs."""
    from palace_amd.fem.fespace import NDHexBoundaryBlock

    ctx = linalg.Context()
    T = _tensors()
    two = lambda a, b: ceed.coefficient_context(3, attr_mat=[0, 1], mat_coeff=[np.asarray(a, float), np.asarray(b, float)])  # noqa: E731
    cm_r, cc_r, cm_i = two(T["mr0"], T["mr1"]), two(T["cr0"], T["cr1"]), two(T["mi0"], T["mi1"])
    mesh = ogrid_cylinder(2, 3)
    mesh.attr[:] = 1 + (np.arange(mesh.ne) % 2)
    nd = NDHexSpace(mesh, 4)
    vgeom = ceed.GeomFactorData(mesh, Q1D)
    nb = int(mesh.boundary_face_mask[mesh.elem_faces].sum())
    blk = NDHexBoundaryBlock(nd, attr=1 + (np.arange(nb) % 2))
    interp, grad, w = blk.tables(Q1D)
    sgeom = ceed.DenseGeomFactorData(blk.elem_nodes, blk.nodes, blk.attr, grad, w)
    sblock = ceed.DenseBlock(ceed.FE_HCURL, nd.ndofs, blk.offsets, interp, None, orients=blk.orients)
    ess = nd.ess_dofs()[::2].copy()  # (part of the boundary: the surface terms touch free and essential dofs)
    n = nd.ndofs
    s_r, s_i = two(0.11, -0.07), two(0.4, 0.25)  # a reactive surface term in the real part, a damping one in the imaginary part

    def volume(op, qf, blob, ev):
        return op.add_integrator(vgeom, nd, qf, blob, ev)

    def surface(op, blob):
        return op.add_dense_integrator(sgeom, sblock, ceed.QF_HCURL_32, blob, ceed.EVAL_INTERP)

    new = lambda: ceed.Operator(n, n)  # noqa: E731
    both = ceed.EVAL_CURL | ceed.EVAL_INTERP
    Ar = surface(volume(new(), ceed.QF_HDIVMASS_33, np.concatenate([cm_r, cc_r]), both), s_r).finalize()
    Ai = surface(volume(new(), ceed.QF_HCURL_33, cm_i, ceed.EVAL_INTERP), s_i).finalize()
    parts = [volume(new(), ceed.QF_HDIVMASS_33, np.concatenate([cm_r, cc_r]), both).finalize(), surface(new(), s_r).finalize(),
             volume(new(), ceed.QF_HCURL_33, cm_i, ceed.EVAL_INTERP).finalize(), surface(new(), s_i).finalize()]
    assert ceed._lib.load().pa_op_complex_fused(Ar.handle, Ai.handle) == 3
    rng = np.random.default_rng(8)
    xr, xi = (_dev(rng.uniform(-1, 1, n)) for _ in range(2))

    def term_by_term(vr, vi):
        def app(o, v):
            y = torch.empty_like(v)
            o.mult(v, y)
            return y

        a_r = lambda v: app(parts[0], v) + app(parts[1], v)  # noqa: E731
        a_i = lambda v: app(parts[2], v) + app(parts[3], v)  # noqa: E731
        return a_r(vr) - a_i(vi), a_i(vr) + a_r(vi)

    for e in (np.zeros(0, np.int32), ess):
        A = linalg.ComplexParOperator(ctx, Ar, Ai, e, linalg.DIAG_ONE)
        yr, yi = torch.empty_like(xr), torch.empty_like(xr)
        A.mult(xr, xi, yr, yi)
        mr, mi = xr.clone(), xi.clone()
        ed = torch.from_numpy(e.astype(np.int64)).cuda()
        mr[ed], mi[ed] = 0.0, 0.0
        wr, wi = term_by_term(mr, mi)
        wr[ed], wi[ed] = xr[ed], xi[ed]
        scale = float(torch.maximum(wr.abs().max(), wi.abs().max()))
        print("surface terms", e.size, float((yr - wr).abs().max()) / scale, float((yi - wi).abs().max()) / scale)
        assert float((yr - wr).abs().max()) < 1e-13 * scale and float((yi - wi).abs().max()) < 1e-13 * scale, e.size
