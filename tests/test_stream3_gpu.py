"""The streaming kernel for three points per direction (pa_nd_hex_stream3.hip: order 2 on its own rule and its p-coarsened
level), selected with PALACE_AMD_STREAM3=1 at operator creation, against the oracle and against the one-shot kernel that stays
the default at this rule.

Criteria as in tests/test_stream5_gpu.py and tests/test_orient_gpu.py: 1e-12 relative l2 against the oracle
(test/unit/test-libceed.cpp:245-282), 1e-13 between two device schedules of one operator, bit equality where the same kernel
computes the same sums, 1e-11 for a smoother against the oracle's recurrence, 1e-9 for solver iterates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import ogrid_cylinder, refine_uniform  # noqa: E402
from tests import util  # noqa: E402
from tests.test_split_gpu import _check_split  # noqa: E402

RTOL = 1e-12
Q1D = 3
SWITCH = "PALACE_AMD_STREAM3"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _nan(n):
    return torch.full((n,), np.nan, dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _with_attr(m):
    """three attributes: the attribute -> material indirection of the per-element coefficients"""
    return type(m)(x=m.x, elem_nodes=m.elem_nodes, attr=(np.arange(m.ne) % 3 + 1).astype(np.int32), bdr_faces=m.bdr_faces,
                   bdr_attr=m.bdr_attr)


def _make(geom, nd, qf, kind):
    _, b_a = util.make_ctx(kind, nattr=3)
    _, b_s = util.make_ctx("scalar", nattr=3)
    if qf == "hdiv":
        return ceed.curlcurl_operator(geom, nd, b_a), b_a
    if qf == "hcurl":
        return ceed.ndmass_operator(geom, nd, b_a), b_a
    return ceed.curlcurlmass_operator(geom, nd, b_s, b_a), np.concatenate([b_s, b_a])


@pytest.fixture(scope="module")
def mesh640(cylinder_mesh):
    m = refine_uniform(cylinder_mesh)
    return type(m)(x=m.x, elem_nodes=m.elem_nodes, attr=(np.arange(m.ne) % 3 + 1).astype(np.int32))


@pytest.fixture(scope="module")
def mesh80(cylinder_mesh):
    return _with_attr(cylinder_mesh)


_ogeom_cache = {}


def _ogeom(mesh):
    """the oracle's geometry factors at three points per direction, once per mesh"""
    if id(mesh) not in _ogeom_cache:
        _ogeom_cache[id(mesh)] = (mesh, util.oracle_geom(mesh, Q1D))
    return _ogeom_cache[id(mesh)][1]


# ---- 1. parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("qf,kind,dstage", [("hdiv", "aniso", None), ("hcurl", "aniso", None), ("hdiv", "scalar", "metric"),
                                            ("hcurl", "scalar", "metric"), ("hdivmass", "scalar", None),
                                            ("hdivmass", "aniso", None)])
@pytest.mark.parametrize("wgx", [None, "1"])
def test_stream3_matches_oracle_and_one_shot(mesh640, monkeypatch, p, qf, kind, dstage, wgx):
    """Packed D (six rows; twelve for anisotropic K + M) and the metric form on 160 batches; with one workgroup per XCD every
    wave walks ten batches (the cross-batch pipeline), with the default launch one."""
    monkeypatch.setenv(SWITCH, "1")
    if dstage:
        monkeypatch.setenv("PALACE_AMD_DSTAGE", dstage)
    if wgx:
        monkeypatch.setenv("PALACE_AMD_STREAM_WGX", wgx)
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    op, blob = _make(geom, nd, qf, kind)
    assert op.streams(), "the streaming kernel was not selected"
    x = np.random.default_rng(3).uniform(-1, 1, nd.ndofs)
    y = op.mult(_dev(x), _nan(nd.ndofs)).cpu().numpy()
    ref = util.oracle_apply_c(nd, _ogeom(mesh), qf, blob, x, Q1D)
    print(f"p = {p} {qf} {kind} {dstage} wgx = {wgx}: against the oracle {_rel(y, ref):.2e}")
    assert _rel(y, ref) < RTOL
    # bit-reproducible (fixed summation order of the run gather)
    assert np.array_equal(op.mult(_dev(x), _new(nd.ndofs)).cpu().numpy(), y)
    # AddMult keeps the one-shot kernel: same operator, different schedule
    y3 = op.add_mult(_dev(x), _dev(ref.copy())).cpu().numpy()
    assert _rel(y3, 2 * ref) < RTOL
    # the same operator created without the switch: the one-shot kernel
    monkeypatch.delenv(SWITCH)
    op1, _ = _make(geom, nd, qf, kind)
    assert not op1.streams()
    y1 = op1.mult(_dev(x), _new(nd.ndofs)).cpu().numpy()
    print(f"    against the one-shot kernel {_rel(y, y1):.2e}")
    assert _rel(y, y1) < 1e-13
    assert op.streams()  # (the first operator keeps the form it was created with)


# ---- 2. the default ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [None, "0"])
def test_stream3_is_opt_in(mesh80, monkeypatch, value):
    """Without the switch (or with it set to 0) orders 1 and 2 at three points keep the one-shot kernel."""
    monkeypatch.delenv(SWITCH, raising=False)
    if value is not None:
        monkeypatch.setenv(SWITCH, value)
    geom = ceed.GeomFactorData(mesh80, Q1D)
    for p in (1, 2):
        nd = NDHexSpace(mesh80, p)
        for qf, kind in (("hdiv", "aniso"), ("hcurl", "aniso"), ("hdivmass", "scalar"), ("hdivmass", "aniso")):
            op, _ = _make(geom, nd, qf, kind)
            assert not op.streams() and not op.supports_split(), (p, qf, kind)


# ---- 3. ragged and tiny meshes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 2])
def test_stream3_ragged_and_tiny_meshes(monkeypatch, p):
    """5 / 10 / 15 / 20 elements: last batches with one, two and three real elements, fewer batches than XCDs."""
    monkeypatch.setenv(SWITCH, "1")
    for n, nz in ((1, 1), (1, 2), (1, 3), (2, 1)):
        mesh = ogrid_cylinder(n, nz)
        nd = NDHexSpace(mesh, p)
        geom = ceed.GeomFactorData(mesh, Q1D)
        og = util.oracle_geom(mesh, Q1D)
        x = np.random.default_rng(7).uniform(-1, 1, nd.ndofs)
        cs, bs = util.make_ctx("scalar")
        blob = po.CoeffCtx().pack()
        for qf, op, bl in (("hdiv", ceed.curlcurl_operator(geom, nd, blob), blob),
                           ("hdivmass", ceed.curlcurlmass_operator(geom, nd, bs, blob), np.concatenate([bs, blob]))):
            assert op.streams()
            y = op.mult(_dev(x), _nan(nd.ndofs)).cpu().numpy()
            ref = util.oracle_apply_c(nd, og, qf, bl, x, Q1D)
            assert _rel(y, ref) < RTOL, (n, nz, mesh.ne, qf, _rel(y, ref))


# ---- 4. essential rows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("policy", ["one", "zero"])
def test_stream3_par_operator_essential_rows(mesh640, monkeypatch, p, policy):
    """ParOperator::Mult (rap.cpp:195-234): essential dofs read as zero inside the kernel, their rows written by the run gather
    (x or 0), bit-exactly."""
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("PALACE_AMD_STREAM_WGX", "2")
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    cm, bm = util.make_ctx("scalar", nattr=3)
    cc, bc = util.make_ctx("identity")
    local = ceed.curlcurlmass_operator(geom, nd, bm, bc)
    assert local.streams()
    ess = nd.ess_dofs()
    pol = linalg.DIAG_ONE if policy == "one" else linalg.DIAG_ZERO
    A = linalg.ParOperator(linalg.Context(), local, ess, pol)
    x = np.random.default_rng(5).uniform(-1, 1, nd.ndofs)
    y = A.mult(_dev(x), _nan(nd.ndofs)).cpu().numpy()
    oracle = util.FastParOperatorOracle(nd, _ogeom(mesh), "hdivmass", np.concatenate([bm, bc]), ess, Q1D, cm, cc,
                                        policy=po.DIAG_ONE if policy == "one" else po.DIAG_ZERO)
    assert _rel(y, oracle.mult(x)) < RTOL
    assert np.array_equal(y[ess], x[ess] if policy == "one" else np.zeros(ess.size))


# ---- 5. the fused Chebyshev step ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 2])
def test_stream3_chebyshev_steps_fused_into_the_gather(mesh640, monkeypatch, p):
    """The smoother step evaluated in the E^T epilogue (pa_op_mult_cheb_step) on the three-point kernel: against the same
    smoother with the step as a vector kernel (PALACE_AMD_FUSED_STEP=0) and against the oracle's recurrence, zero and non-zero
    initial guess."""
    monkeypatch.setenv(SWITCH, "1")
    mesh = mesh640
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    cm, bm = util.make_ctx("scalar", nattr=3)
    cc, bc = util.make_ctx("identity")
    local = ceed.curlcurlmass_operator(geom, nd, bm, bc)
    assert local.streams()
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
    y = S.mult(_dev(b), _new(n)).cpu().numpy()
    y0 = S0.mult(_dev(b), _new(n)).cpu().numpy()
    z = S.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    z0 = S0.mult(_dev(b), _dev(g.copy()), initial_guess=True).cpu().numpy()
    assert _rel(y, y0) < 1e-13 and _rel(z, z0) < 1e-13
    oracle = util.FastParOperatorOracle(nd, _ogeom(mesh), "hdivmass", np.concatenate([bm, bc]), ess, Q1D, cm, cc)
    oracle._diag = A.assemble_diagonal(_new(n)).cpu().numpy()
    o = po.ChebyshevOracle(oracle, 4, lambda_max=S.lambda_max())
    assert _rel(y, o.mult2(b, None, False)) < 1e-11 and _rel(z, o.mult2(b, g.copy(), True)) < 1e-11


# ---- 6. split vectors --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["curl", "curlmass", "mass"])
@pytest.mark.parametrize("p", [1, 2])
def test_stream3_split_apply_equals_plain_apply(cylinder_mesh, monkeypatch, p, kind):
    """pa_op_mult_split on the three-point kernels: split points n, 0.7 n and 1, the ghost input in the second of two buffers
    with the first one poisoned, both essential policies; bit-equal to mult (tests/test_split_gpu.py: _check_split)."""
    monkeypatch.setenv(SWITCH, "1")
    mesh = cylinder_mesh
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    mass = ceed.coefficient_context(3, attr_mat=[0] * int(mesh.attr.max()), mat_coeff=[np.array([2.08])])
    ident = ceed.coefficient_context(3)
    make = {"curl": lambda: ceed.curlcurl_operator(geom, nd, ident),
            "curlmass": lambda: ceed.curlcurlmass_operator(geom, nd, mass, ident),
            "mass": lambda: ceed.ndmass_operator(geom, nd, mass)}[kind]
    op = make()
    assert op.streams() and op.supports_split()
    _check_split(make, nd.ndofs, p)


# ---- 7. rotated elements -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 2])
def test_stream3_rotated_elements(mesh80, monkeypatch, p):
    """Every element handed over in one of the 24 rotations of the reference cube (tests/test_orient_gpu.py): K, M, K + M with a
    scalar and a symmetric tensor."""
    monkeypatch.setenv(SWITCH, "1")
    mesh = util.rotate_elements(mesh80, util.seeded_rotations(mesh80.ne, 24))
    nd = NDHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, Q1D)
    og = util.oracle_geom(mesh, Q1D)
    x = np.random.default_rng(100 * p + Q1D).uniform(-1, 1, nd.ndofs)
    for kind in ("scalar", "aniso"):
        ck, bk = util.make_ctx(kind, nattr=3)
        for qf in ("hdiv", "hcurl", "hdivmass"):
            if qf == "hdiv":
                op, blob, cs = ceed.curlcurl_operator(geom, nd, bk), bk, (ck, None)
            elif qf == "hcurl":
                op, blob, cs = ceed.ndmass_operator(geom, nd, bk), bk, (ck, None)
            else:
                op, blob, cs = ceed.curlcurlmass_operator(geom, nd, bk, bk), np.concatenate([bk, bk]), (ck, ck)
            assert op.streams(), (kind, qf)
            ref = util.oracle_apply_c(nd, og, qf, blob, x, Q1D)
            y = op.mult(_dev(x), _nan(nd.ndofs)).cpu().numpy()
            assert _rel(y, ref) < RTOL, (kind, qf, _rel(y, ref))
            assert np.array_equal(op.mult(_dev(x), _new(nd.ndofs)).cpu().numpy(), y)
            d = op.assemble_diagonal(_new(nd.ndofs)).cpu().numpy()
            assert _rel(d, util.oracle_operator(nd, og, qf, cs[0], cs[1], Q1D).diagonal()) < RTOL, (kind, qf, "diagonal")


# ---- 8. a numbering the index refuses ------------------------------------------------------------------------------------------

def test_stream3_refused_numbering_keeps_the_one_shot_kernel(mesh80, monkeypatch):
    """A random permutation of the dofs: every entry of an element is a run of its own, pack_index refuses and the operator
    keeps the one-shot kernel, switch or not."""
    monkeypatch.setenv(SWITCH, "1")
    p = 2
    natural = NDHexSpace(mesh80, p)
    n = natural.ndofs
    perm = np.random.default_rng(5).permutation(n)
    space = util.renumbered(natural, perm)
    geom = ceed.GeomFactorData(mesh80, Q1D)
    og = _ogeom(mesh80)
    ck, bk = util.make_ctx("aniso", nattr=3)
    op = ceed.curlcurlmass_operator(geom, space, bk, bk)
    assert not op.streams()
    assert ceed.curlcurlmass_operator(geom, natural, bk, bk).streams()  # (the numbering, not the operator, is what is refused)
    blob = np.concatenate([bk, bk])
    x = np.random.default_rng(42).uniform(-1, 1, n)
    ref = util.oracle_apply_c(space, og, "hdivmass", blob, x, Q1D)
    assert _rel(op.mult(_dev(x), _nan(n)).cpu().numpy(), ref) < RTOL
    y0 = np.random.default_rng(7).uniform(-1, 1, n)
    assert _rel(op.add_mult(_dev(x), _dev(y0.copy())).cpu().numpy(), y0 + ref) < RTOL
    d = op.assemble_diagonal(_new(n)).cpu().numpy()
    assert _rel(d, util.oracle_operator(space, og, "hdivmass", ck, ck, Q1D).diagonal()) < RTOL


# ---- 9. the coarsened level and a solve ----------------------------------------------------------------------------------------

def _levels(mesh, geom):
    cm, bm = util.make_ctx("scalar", nattr=3)
    cc, bc = util.make_ctx("identity")
    spaces = [NDHexSpace(mesh, 1), NDHexSpace(mesh, 2)]
    fine = ceed.curlcurlmass_operator(geom, spaces[1], bm, bc)
    return spaces, [fine.coarsen(geom, spaces[0]), fine], np.concatenate([bm, bc])


def test_stream3_coarsened_level(mesh640, monkeypatch):
    """fine.coarsen(order-1 space) of an order-2 operator shares the fine q-data and streams at (1, 3)."""
    monkeypatch.setenv(SWITCH, "1")
    geom = ceed.GeomFactorData(mesh640, Q1D)
    spaces, local, blob = _levels(mesh640, geom)
    assert local[0].streams() and local[1].streams()
    nd = spaces[0]
    x = np.random.default_rng(11).uniform(-1, 1, nd.ndofs)
    y = local[0].mult(_dev(x), _nan(nd.ndofs)).cpu().numpy()
    assert _rel(y, util.oracle_apply_c(nd, _ogeom(mesh640), "hdivmass", blob, x, Q1D)) < RTOL


def test_stream3_pcg_p_multigrid_same_iterations(mesh640, monkeypatch):
    """PCG + p-multigrid (1, 2) to 1e-10: the same number of iterations with and without the switch, the same solution to
    1e-9."""
    geom = ceed.GeomFactorData(mesh640, Q1D)
    results = []
    for on in (True, False):
        if on:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH)
        spaces, local, _ = _levels(mesh640, geom)
        assert [op.streams() for op in local] == [on, on]
        ctx = linalg.Context()
        A = [linalg.ParOperator(ctx, op, s.ess_dofs(), linalg.DIAG_ONE) for op, s in zip(local, spaces)]
        P = [linalg.Interp(ctx, spaces[0], spaces[1])]
        B = linalg.gmg(ctx, A, P, linalg.chebyshev(ctx, A[0], 4), cheby_order=4)
        assert B.fused_step(1) == on
        K = linalg.cg(ctx, A[1], B, rel_tol=1e-10, max_it=200)
        n = spaces[1].ndofs
        b = A[1].mult(torch.ones(n, dtype=torch.float64, device="cuda"), _new(n))
        b[torch.from_numpy(spaces[1].ess_dofs().astype(np.int64)).cuda()] = 0.0
        x = K.mult(b, _new(n)).cpu().numpy()
        st = K.stats()
        assert st["converged"]
        results.append((st["iterations"], x))
        del K, B, P, A, local
    print(f"PCG + p-multigrid (1, 2), 640 elements: {results[0][0]} / {results[1][0]} iterations with / without the switch, "
          f"solutions differ by {_rel(results[0][1], results[1][1]):.2e}")
    assert results[0][0] == results[1][0]
    assert _rel(results[0][1], results[1][1]) < 1e-9


# ---- 10. no complex form -------------------------------------------------------------------------------------------------------

def test_stream3_claims_no_one_pass_complex_form(mesh80, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    geom = ceed.GeomFactorData(mesh80, Q1D)
    nd = NDHexSpace(mesh80, 2)
    _, bs = util.make_ctx("scalar", nattr=3)
    _, ba = util.make_ctx("aniso", nattr=3)
    _, bi = util.make_ctx("identity")
    for Ar, Ai in ((ceed.curlcurlmass_operator(geom, nd, bs, bi), ceed.ndmass_operator(geom, nd, bs)),
                   (ceed.curlcurlmass_operator(geom, nd, bs, ba), ceed.ndmass_operator(geom, nd, ba))):
        assert Ar.streams()
        assert ceed._lib.load().pa_op_complex_fused(Ar.handle, Ai.handle) == 0
