"""Every option of the algebraic cycles (palace_amd/csrc/amg_solver.hip: AmgSolver, AmsSolver, cheb4 in its fused and unfused
form) against the restated cycle (oracle: amg_vcycle, ams_cycle) on the library's own hierarchy: smoother orders 1, 3 and 4 (the
buffer rotation of the fused form differs for order 1, 2, 3 and >= 4), the aggregation threshold of the flux projectors, a last
level that keeps the smoother instead of the direct solve, several AMS cycles per application, an application from an initial
iterate, both `singular` settings -- and AMS on tetrahedra and on triangles (dim = 2), which the suite otherwise checks only
through "the outer solve converges".  Every case runs with PALACE_AMD_FUSED_STEP_CSR "1" and "0" at creation: both forms against
the restatement (1e-10 AMG, 1e-9 AMS, the bounds of tests/test_ams_gpu.py) and against each other (1e-12); zero-guess
applications are symmetric, c . B b = b . B c."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import H1HexSpace, NDHexSpace, lowest_order_gradient, vertex_coordinates  # noqa: E402
from palace_amd.fem.mesh import ogrid_cylinder  # noqa: E402
from oracle import palace_oracle as po  # noqa: E402

AMG_TOL, AMS_TOL, FORM_TOL = 1e-10, 1e-9, 1e-12
TET_M = 2   # smallest cube_tet_mesh(m) / unit-square grid whose two auxiliary hierarchies have two levels at amg_coarse_size=20
TRI_N = 4   # (asserted below, with the next smaller one falling short)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _eliminated(Asp, ess):
    import scipy.sparse as sp

    keep = np.ones(Asp.shape[0])
    keep[ess] = 0.0
    D = sp.diags(keep)
    return (D @ Asp @ D + sp.diags(1.0 - keep)).tocsr()


def _apply(B, b, x0=None):
    n = b.size
    if x0 is None:
        return B.mult(_dev(b), torch.full((n,), np.nan, dtype=torch.float64, device="cuda")).cpu().numpy()
    return B.mult(_dev(b), _dev(x0.copy()), initial_guess=True).cpu().numpy()


def _both_forms(monkeypatch, create):
    out = {}
    for form in ("1", "0"):
        monkeypatch.setenv("PALACE_AMD_FUSED_STEP_CSR", form)
        out[form] = create()
    monkeypatch.delenv("PALACE_AMD_FUSED_STEP_CSR")
    return out


def _check(label, ys, ref, tol, zs=None, b=None, c=None):
    """ys / zs: {form: B b} / {form: B c}; prints every figure before it asserts."""
    e1, e0, ef = _rel(ys["1"], ref), _rel(ys["0"], ref), _rel(ys["1"], ys["0"])
    print(f"{label}: fused vs restated {e1:.3e}, unfused vs restated {e0:.3e}, fused vs unfused {ef:.3e}")
    assert np.all(np.isfinite(ys["1"])) and np.all(np.isfinite(ys["0"]))
    assert e1 < tol and e0 < tol and ef < FORM_TOL, (label, e1, e0, ef)
    if zs is not None:
        for form in ("1", "0"):
            lhs, rhs = c @ ys[form], b @ zs[form]
            print(f"{label}: form {form} symmetry defect {abs(lhs - rhs) / abs(lhs):.3e}")
            assert abs(lhs - rhs) < tol * abs(lhs) and b @ ys[form] > 0, (label, form, lhs, rhs)


@pytest.fixture(scope="module")
def hexes():
    mesh = ogrid_cylinder(4, 10)  # 800 hexahedra
    geom = ceed.GeomFactorData(mesh, 2)
    h1, nd = H1HexSpace(mesh, 1), NDHexSpace(mesh, 1)
    mass = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[np.array([2.08])])
    ctx = linalg.Context()
    # order-1 H1 diffusion with Dirichlet rows
    op_h1 = ceed.diffusion_operator(geom, h1, mass)
    # order-1 Nedelec curl-curl + mass
    op_nd = ceed.curlcurlmass_operator(geom, nd, mass, ceed.coefficient_context(3))
    ess_nd = nd.ess_dofs()
    G, X = lowest_order_gradient(h1, nd), vertex_coordinates(h1)
    flag = np.zeros(nd.ndofs, dtype=bool)
    flag[ess_nd] = True
    Gb, Pi = po.ams_nodal_interpolation(G, X, flag)
    return dict(ctx=ctx, h1=h1, nd=nd, keep=(mesh, geom, op_h1, op_nd), csr_h1=op_h1.full_assemble_device(), ess_h1=h1.ess_dofs(),
                csr_nd=op_nd.full_assemble_device(), ess_nd=ess_nd, Asp_nd=_eliminated(op_nd.full_assemble(), ess_nd), G=G, X=X, Gb=Gb,
                Pi=Pi)


AMG_CASES = {
    "order1": dict(smooth_order=1, coarse_size=60),
    "order3": dict(smooth_order=3, coarse_size=60),
    "order4": dict(smooth_order=4, coarse_size=60),
    "theta0.8": dict(theta=0.8, coarse_size=60),
    # two levels, the second one far above 4 x coarse_size rows: it keeps the smoother (one zero-guess smoothing, three more)
    "smoothed_last_level": dict(max_levels=2, coarse_size=5),
    "smoothed_last_level_order3": dict(max_levels=2, coarse_size=5, smooth_order=3),
}


@pytest.mark.parametrize("case", list(AMG_CASES))
def test_amg_cycle_options_against_the_restated_cycle(hexes, monkeypatch, case):
    opts = AMG_CASES[case]
    ctx, n = hexes["ctx"], hexes["h1"].ndofs
    Bs = _both_forms(monkeypatch, lambda: linalg.amg(ctx, hexes["csr_h1"], hexes["ess_h1"], **opts))
    A_l, P_l, cinv = linalg.amg_hierarchy(Bs["1"])
    A_0, P_0, cinv_0 = linalg.amg_hierarchy(Bs["0"])
    assert [a.shape for a in A_l] == [a.shape for a in A_0] and (cinv is None) == (cinv_0 is None)
    if case.startswith("smoothed_last_level"):
        assert cinv is None and len(A_l) == 2 and A_l[-1].shape[0] > 4 * opts["coarse_size"]
    elif case == "theta0.8":  # (nothing on this matrix is that strongly tied: no coarsening at all, the one level is smoothed four times)
        assert cinv is None
    else:
        assert cinv is not None and len(A_l) >= 2
    print(f"{case}: levels {[a.shape[0] for a in A_l]}")
    rng = np.random.default_rng(10)
    b, c = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    order = opts.get("smooth_order", 2)
    ys = {f: _apply(B, b) for f, B in Bs.items()}
    zs = {f: _apply(B, c) for f, B in Bs.items()}
    _check(case, ys, po.amg_vcycle(A_l, P_l, cinv, b, order=order), AMG_TOL, zs, b, c)


def _ams_reference(B, Asp, Gb, Pi, b, amg_order, **kw):
    hp = linalg.amg_hierarchy(B, 2)
    solve_pi = lambda r: po.amg_vcycle(*hp, r, order=amg_order)  # noqa: E731
    solve_g = None
    if not kw.get("singular", False):
        hg = linalg.amg_hierarchy(B, 1)
        solve_g = lambda r: po.amg_vcycle(*hg, r, order=amg_order)  # noqa: E731
    return po.ams_cycle(Asp, Gb, Pi, solve_g, solve_pi, b, **kw)


AMS_CASES = {
    "orders_1_1": dict(smooth_order=1, amg_smooth_order=1),
    "orders_3_3": dict(smooth_order=3, amg_smooth_order=3),
    "orders_1_3_two_cycles": dict(smooth_order=1, amg_smooth_order=3, cycle_it=2),
    "orders_3_1_two_cycles_singular": dict(smooth_order=3, amg_smooth_order=1, cycle_it=2, singular=True),
    "two_cycles": dict(cycle_it=2),
    "two_cycles_singular": dict(cycle_it=2, singular=True),
    "initial_guess": dict(guess=True),
    "initial_guess_singular": dict(guess=True, singular=True),
    "initial_guess_order3_two_cycles": dict(guess=True, smooth_order=3, cycle_it=2),
    "theta0.8": dict(amg_theta=0.8),
}


@pytest.mark.parametrize("case", list(AMS_CASES))
def test_ams_cycle_options_against_the_restated_cycle(hexes, monkeypatch, case):
    opts = dict(AMS_CASES[case])
    guess = opts.pop("guess", False)
    ctx, n, ess = hexes["ctx"], hexes["nd"].ndofs, hexes["ess_nd"]
    Bs = _both_forms(monkeypatch, lambda: linalg.ams(ctx, hexes["csr_nd"], ess, hexes["G"], hexes["X"], amg_coarse_size=60, **opts))
    levels = [[a.shape[0] for a in linalg.amg_hierarchy(Bs["1"], w)[0]] for w in ((2,) if opts.get("singular") else (1, 2))]
    print(f"{case}: auxiliary levels {levels}")
    assert "amg_theta" in opts or all(len(lv) >= 2 for lv in levels)
    rng = np.random.default_rng(11)
    b, c, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b[ess] = c[ess] = x0[ess] = 0.0
    kw = dict(order=opts.get("smooth_order", 2), singular=opts.get("singular", False), cycle_it=opts.get("cycle_it", 1))
    ref = _ams_reference(Bs["1"], hexes["Asp_nd"], hexes["Gb"], hexes["Pi"], b, opts.get("amg_smooth_order", 2), x0=x0 if guess else None, **kw)
    ys = {f: _apply(B, b, x0 if guess else None) for f, B in Bs.items()}
    assert all(np.all(y[ess] == 0.0) for y in ys.values())
    zs = None if guess else {f: _apply(B, c) for f, B in Bs.items()}
    _check(case, ys, ref, AMS_TOL, zs, b, c)


def _tet_problem(m):
    from palace_amd.fem import tet

    tm = tet.cube_tet_mesh(m)
    nd, h1 = tet.NDTetSpace(tm, 1), tet.H1TetSpace(tm, 1)
    pts, wts = tet.default_tet_rule(1)
    interp, curl = nd.elem.tables(pts)
    geom = ceed.DenseGeomFactorData(tm.elem_nodes, tm.nodes, tm.attr, tm.geometry_grad_table(pts), wts)
    kw = dict(orients=nd.orients) if nd.diagonal_transform else dict(curl_orients=nd.curl_orients)
    block = ceed.DenseBlock(ceed.FE_HCURL, nd.ndofs, nd.offsets, interp, curl, **kw)
    mass = ceed.coefficient_context(3, attr_mat=[0] * int(tm.attr.max()), mat_coeff=[np.array([2.08])])
    op = ceed.Operator(nd.ndofs, nd.ndofs).add_dense_integrator(geom, block, ceed.QF_HDIVMASS_33, np.concatenate([mass, ceed.coefficient_context(3)]),
                                                               ceed.EVAL_CURL | ceed.EVAL_INTERP).finalize()
    return op, nd.ess_dofs(), tet.lowest_order_gradient(h1, nd), tet.vertex_coordinates(h1), (tm, geom, block)


def _tri_problem(n):
    from palace_amd.fem import tri

    g = np.arange(n + 1) / n
    verts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    verts = verts + 0.15 / n * np.sin(7.0 * verts[:, ::-1] + 1.0) * (verts * (1 - verts))  # (interior vertices moved: no two elements alike)
    v = lambda i, j: i * (n + 1) + j  # noqa: E731
    tris = [t for i in range(n) for j in range(n) for t in ((v(i, j), v(i + 1, j), v(i + 1, j + 1)), (v(i, j), v(i + 1, j + 1), v(i, j + 1)))]
    tm = tri.TriMesh(verts, np.array(tris))
    nd, h1 = tri.NDTriSpace(tm, 1), tri.H1TriSpace(tm, 1)
    pts, wts = tri.tri_quadrature(2)
    interp, curl = nd.elem.tables(pts)
    geom = ceed.DenseGeomFactorData(tm.elem_nodes, tm.nodes, tm.attr, tm.geometry_grad_table(pts), wts)
    block = ceed.DenseBlock(ceed.FE_HCURL, nd.ndofs, nd.offsets, interp, curl, orients=nd.orients)
    mass = ceed.coefficient_context(2, attr_mat=[0], mat_coeff=[np.array([2.08])])
    op = ceed.Operator(nd.ndofs, nd.ndofs).add_dense_integrator(geom, block, ceed.QF_HDIVMASS_22, np.concatenate([mass, ceed.coefficient_context(1)]),
                                                               ceed.EVAL_CURL | ceed.EVAL_INTERP | ceed.EVAL_WEIGHT).finalize()
    return op, nd.ess_dofs(), tri.lowest_order_gradient(h1, nd), tri.vertex_coordinates(h1), (tm, geom, block)


def _aux_levels(B):
    return min(len(linalg.amg_hierarchy(B, w)[0]) for w in (1, 2))


@pytest.mark.parametrize("family", ["tet", "tri"])
def test_ams_cycle_on_simplices_against_the_restated_cycle(monkeypatch, family):
    """Order-1 curl-curl + mass on tetrahedra and on triangles (dim = 2), default options, singular false: the smallest mesh of
    the family whose gradient- and nodal-space hierarchies both have two levels at amg_coarse_size=20."""
    make, size = (_tet_problem, TET_M) if family == "tet" else (_tri_problem, TRI_N)
    ctx = linalg.Context()
    # the next smaller mesh falls short of two levels in one of the two auxiliary spaces
    op_s, ess_s, G_s, X_s, keep_s = make(size - 1)
    assert _aux_levels(linalg.ams(ctx, op_s.full_assemble_device(), ess_s, G_s, X_s, amg_coarse_size=20)) < 2
    op, ess, G, X, keep = make(size)
    assert X.shape[1] == (3 if family == "tet" else 2)
    n = op.full_assemble().shape[0]
    csr = op.full_assemble_device()
    Bs = _both_forms(monkeypatch, lambda: linalg.ams(ctx, csr, ess, G, X, amg_coarse_size=20))
    assert _aux_levels(Bs["1"]) >= 2 and _aux_levels(Bs["0"]) >= 2
    Asp = _eliminated(op.full_assemble(), ess)
    flag = np.zeros(n, dtype=bool)
    flag[ess] = True
    Gb, Pi = po.ams_nodal_interpolation(G, X, flag)
    rng = np.random.default_rng(12)
    b, c = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b[ess] = c[ess] = 0.0
    ref = _ams_reference(Bs["1"], Asp, Gb, Pi, b, 2)
    ys = {f: _apply(B, b) for f, B in Bs.items()}
    zs = {f: _apply(B, c) for f, B in Bs.items()}
    assert all(np.all(y[ess] == 0.0) for y in ys.values())
    _check(family, ys, ref, AMS_TOL, zs, b, c)
