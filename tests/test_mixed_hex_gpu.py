"""Sum-factorised two-space forms on tensor-product hexahedra (palace_amd/csrc/pa_mixed_hex.hip through pa_op_add_sub_mixed and
pa_error_op_create_tensor): the mixed mass (v, C u) between a Nedelec and a Raviart-Thomas space of the same order, either way
round, and the element error integrator of the flux error estimators (linalg/errorestimator.cpp) -- against the oracle, against
the dense two-space path (pa_mixed.hip) and as the estimator procedure at the orders the dense path cannot reach.  The meshes
are those of tests/rthex_util.py: every element rotated, two attributes."""
import ctypes as C

import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import util

pytestmark = pytest.mark.gpu

PQ = [(1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4), (1, 5), (2, 5), (3, 5), (4, 5)]  # PA_HEX_PQ_LIST
REL = 1e-12  # the project's operator-level tolerance
_cache = {}


def _element_order(geom):
    from palace_amd import lib

    order = np.zeros(geom.mesh.ne, dtype=np.int32)
    lib.check(lib.load().pa_geom_element_order(geom.handle, order.ctypes.data_as(C.c_void_p)))
    return order


def _mesh(kind):
    """The fixture of tests/rthex_util.py.  The error integrator walks the geometry data's internal element order and writes
    in the caller's: on cyl80 the two must differ, so if the library keeps the fixture's order its elements are first renumbered
    with a seeded permutation."""
    if ("mesh", kind) not in _cache:
        from palace_amd import ceed
        from palace_amd.fem.mesh import HexMesh

        m = ru.mesh(kind)
        if kind == "cyl80" and np.array_equal(_element_order(ceed.GeomFactorData(m, 2)), np.arange(m.ne)):
            perm = np.random.default_rng(80).permutation(m.ne)
            m = HexMesh(x=m.x, elem_nodes=m.elem_nodes[perm], attr=m.attr[perm], bdr_faces=m.bdr_faces, bdr_attr=m.bdr_attr)
            m.check()
        _cache["mesh", kind] = m
    return _cache["mesh", kind]


def _spaces(kind, p):
    """(Nedelec space, Raviart-Thomas space)."""
    if ("sp", kind, p) not in _cache:
        from palace_amd.fem import rthex
        from palace_amd.fem.fespace import NDHexSpace

        m = _mesh(kind)
        _cache["sp", kind, p] = (NDHexSpace(m, p), ru.space(kind, p) if m is ru.mesh(kind) else rthex.RTHexSpace(m, p))
    return _cache["sp", kind, p]


def _geom(kind, q1d):
    if ("geom", kind, q1d) not in _cache:
        from palace_amd import ceed

        _cache["geom", kind, q1d] = ceed.GeomFactorData(_mesh(kind), q1d)
    return _cache["geom", kind, q1d]


def _ogeom(kind, q1d):
    if ("ogeom", kind, q1d) not in _cache:
        m = _mesh(kind)
        _cache["ogeom", kind, q1d] = ru.ogeom(kind, q1d) if m is ru.mesh(kind) else util.oracle_geom(m, q1d)
    return _cache["ogeom", kind, q1d]


def _oracles(kind, p, q1d):
    """CeedOperatorOracle objects of the two spaces (MixedSpaceOracle reads their restrictions and value tables)."""
    if ("orc", kind, p, q1d) not in _cache:
        nd, sp = _spaces(kind, p)
        og = _ogeom(kind, q1d)
        off, ori = nd.native_restriction()
        nint, ncurl = util.dense_tables(nd, q1d)
        nint, ncurl = np.asarray(nint).reshape(3, -1, nd.P), np.asarray(ncurl).reshape(3, -1, nd.P)
        rint, _ = ru.tables(p, q1d)
        ndo = po.CeedOperatorOracle(nd.ndofs, off, ori, nint, ncurl, og, po.QF_HCURL, None)
        rto = po.CeedOperatorOracle(sp.ndofs, sp.elem_dof_lex, sp.elem_sign_lex < 0, rint, rint, og, po.QF_HDIV, None)
        _cache["orc", kind, p, q1d] = (ndo, rto)
    return _cache["orc", kind, p, q1d]


def _sides(kind, p, q1d, nd_first):
    """((space, oracle) of the first side, the same of the second)."""
    (nd, sp), (ndo, rto) = _spaces(kind, p), _oracles(kind, p, q1d)
    return ((nd, ndo), (sp, rto)) if nd_first else ((sp, rto), (nd, ndo))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mult(op, x, transpose=False):
    import torch

    y = torch.full((op.width if transpose else op.height,), 7.0, dtype=torch.float64, device="cuda")  # Mult overwrites
    (op.mult_transpose if transpose else op.mult)(_dev(x), y)
    return y.cpu().numpy()


def _relerr(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


def _mass_reference(kind, p, q1d, nd_trial, ctx_name):
    """(x, (v, C u) of the oracle), cached: several tests read it."""
    key = ("mass", kind, p, q1d, nd_trial, ctx_name)
    if key not in _cache:
        (tr, tro), (te, teo) = _sides(kind, p, q1d, nd_trial)
        x = ru.vector(tr.ndofs, 100 * p + q1d + int(nd_trial))
        qfo = po.QF_HCURLHDIV if nd_trial else po.QF_HDIVHCURL
        ref = po.MixedSpaceOracle(tro, teo, _ogeom(kind, q1d), qfo, ru.mass_ctx(ctx_name)).apply_add(x, np.zeros(te.ndofs))
        ref.setflags(write=False)
        _cache[key] = (x, ref)
    return _cache[key]


def _mass_operator(kind, p, q1d, nd_trial, ctx_name="nonsym"):
    from palace_amd import ceed

    (tr, _), (te, _) = _sides(kind, p, q1d, nd_trial)
    return ceed.mixedmass_operator(_geom(kind, q1d), tr, te, ru.mass_ctx(ctx_name).pack())


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("nd_trial", [True, False], ids=["hcurlhdiv", "hdivhcurl"])
@pytest.mark.parametrize("p,q1d", PQ)
def test_mixed_mass_against_oracle(p, q1d, nd_trial, kind):
    """mult and add_mult into a non-zero y; a non-symmetric material exposes a swapped factor order."""
    op = _mass_operator(kind, p, q1d, nd_trial)
    x, ref = _mass_reference(kind, p, q1d, nd_trial, "nonsym")
    e = _relerr(_mult(op, x), ref)
    print(f"mult {e:.2e}")
    assert e < REL
    y0 = ru.vector(ref.size, 5)
    y = _dev(y0)
    op.add_mult(_dev(x), y)
    e = np.abs(y.cpu().numpy() - (y0 + ref)).max() / np.abs(ref).max()
    print(f"add_mult {e:.2e}")
    assert e < REL
    assert not op.is_symmetric()
    nd, sp = _spaces(kind, p)
    assert op.algorithmic_bytes() == nd.mesh.ne * (q1d**3 * 11 * 8 + (nd.P + sp.P) * 6) + 8.0 * (nd.ndofs + sp.ndofs)


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("nd_trial", [True, False], ids=["hcurlhdiv", "hdivhcurl"])
@pytest.mark.parametrize("p,q1d", PQ)
def test_mixed_mass_transpose(p, q1d, nd_trial, kind):
    """A^T of the operator with C is the other QFunction's operator with every material matrix transposed (the identity holds
    on the oracle to 2e-15)."""
    op = _mass_operator(kind, p, q1d, nd_trial)
    other = _mass_operator(kind, p, q1d, not nd_trial, "nonsym_t")
    z = ru.vector(op.height, 17)
    e = _relerr(_mult(op, z, transpose=True), _mult(other, z))
    print(f"transpose {e:.2e}")
    assert e < 1e-13
    _, ref = _mass_reference(kind, p, q1d, nd_trial, "nonsym")  # ... and not merely both wrong in the same way
    x, _ = _mass_reference(kind, p, q1d, nd_trial, "nonsym")
    assert abs(z @ ref - _mult(op, z, transpose=True) @ x) < 1e-12 * abs(z @ ref)


def _dense_setup(p):
    """The dense two-space path on cyl80, as tests/test_estimator_gpu.py::_hex_setup builds it."""
    if ("dense", p) not in _cache:
        from palace_amd import ceed

        kind, q1d = "cyl80", p + 1
        mesh = _mesh(kind)
        nd, sp = _spaces(kind, p)
        ndo, rto = _oracles(kind, p, q1d)
        _, wts = po.hex_quadrature(q1d)
        dgeom = ceed.DenseGeomFactorData(mesh.elem_nodes, mesh.x, mesh.attr, po.mesh_q2_grad_table(q1d), wts)
        ndb = ceed.DenseBlock(ceed.FE_HCURL, nd.ndofs, ndo.off, ndo.interp, ndo.deriv, orients=ndo.sgn < 0)
        rtb = ceed.DenseBlock(ceed.FE_HDIV, sp.ndofs, sp.elem_dof_lex, rto.interp, None, orients=sp.elem_sign_lex < 0)
        _cache["dense", p] = (dgeom, ndb, rtb)
    return _cache["dense", p]


@pytest.mark.parametrize("p", [1, 2])
def test_same_numbers_as_dense_path(p):
    import torch

    from palace_amd import ceed

    kind, q1d = "cyl80", p + 1
    dgeom, ndb, rtb = _dense_setup(p)
    nd, sp = _spaces(kind, p)
    _, b_ns = util.make_ctx("nonsym", 2)
    _, b_an = util.make_ctx("aniso", 2)
    for nd_first in (True, False):
        (s1, _), (s2, _) = _sides(kind, p, q1d, nd_first)
        d1, d2 = (ndb, rtb) if nd_first else (rtb, ndb)
        qf = ceed.QF_HCURLHDIV_33 if nd_first else ceed.QF_HDIVHCURL_33
        dense = ceed.Operator(d2.lsize, d1.lsize).add_dense_mixed_integrator(dgeom, d1, d2, qf, b_ns).finalize()
        x = ru.vector(s1.ndofs, 3)
        e = _relerr(_mult(_mass_operator(kind, p, q1d, nd_first), x), _mult(dense, x))
        print(f"mass {e:.2e}")
        assert e < 1e-13
        qfe = ceed.QF_HCURLHDIV_ERROR_33 if nd_first else ceed.QF_HDIVHCURL_ERROR_33
        pair = np.concatenate([b_an, b_ns])
        u1, u2 = _dev(ru.vector(s1.ndofs, 4)), _dev(ru.vector(s2.ndofs, 6))
        est = []
        for integ in (ceed.HexElementErrorIntegrator(_geom(kind, q1d), s1, s2, qfe, pair),
                      ceed.ElementErrorIntegrator(dgeom, d1, d2, qfe, pair)):
            assert integ.ne == nd.mesh.ne
            est.append(integ.apply_add(u1, u2, torch.zeros(integ.ne, dtype=torch.float64, device="cuda")).cpu().numpy())
        e = _relerr(est[0], est[1])
        print(f"error {e:.2e}")
        assert e < 1e-13


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("nd_first", [True, False], ids=["hcurlhdiv_error", "hdivhcurl_error"])
@pytest.mark.parametrize("p,q1d", PQ)
def test_element_error_against_oracle(p, q1d, nd_first, kind):
    """ApplyAdd into a random non-negative vector; the estimates are in the caller's element order although the kernel walks
    the geometry data's own."""
    from palace_amd import ceed

    geom = _geom(kind, q1d)
    if kind == "cyl80":
        assert not np.array_equal(_element_order(geom), np.arange(geom.mesh.ne))
    (s1, o1), (s2, o2) = _sides(kind, p, q1d, nd_first)
    c_an, b_an = util.make_ctx("aniso", 2)
    c_ns, b_ns = util.make_ctx("nonsym", 2)
    qf, qfo = ((ceed.QF_HCURLHDIV_ERROR_33, po.QF_HCURLHDIV_ERROR) if nd_first else
               (ceed.QF_HDIVHCURL_ERROR_33, po.QF_HDIVHCURL_ERROR))
    integ = ceed.HexElementErrorIntegrator(geom, s1, s2, qf, np.concatenate([b_an, b_ns]))
    rng = np.random.default_rng(10 * p + q1d)
    u1, u2 = rng.uniform(-1, 1, s1.ndofs), rng.uniform(-1, 1, s2.ndofs)
    e0 = rng.uniform(0, 1, integ.ne)
    ref = po.MixedSpaceOracle(o1, o2, _ogeom(kind, q1d), qfo, c_an, c_ns).error_add(u1, u2, e0.copy())
    est = _dev(e0.copy())
    integ.apply_add(_dev(u1), _dev(u2), est)
    e = _relerr(est.cpu().numpy(), ref)
    print(f"error {e:.2e}")
    assert e < REL
    assert (ref - e0).min() > 0


@pytest.mark.parametrize("p,q1d", [(3, 4), (4, 5)])
def test_bit_reproducible(p, q1d):
    import torch

    from palace_amd import ceed

    kind = "cyl80"
    _, b_an = util.make_ctx("aniso", 2)
    _, b_ns = util.make_ctx("nonsym", 2)
    for nd_first in (True, False):
        (s1, _), (s2, _) = _sides(kind, p, q1d, nd_first)
        op = _mass_operator(kind, p, q1d, nd_first)
        x = ru.vector(s1.ndofs, 8)
        assert np.array_equal(_mult(op, x), _mult(op, x))
        qf = ceed.QF_HCURLHDIV_ERROR_33 if nd_first else ceed.QF_HDIVHCURL_ERROR_33
        integ = ceed.HexElementErrorIntegrator(_geom(kind, q1d), s1, s2, qf, np.concatenate([b_an, b_ns]))
        u1, u2 = _dev(x), _dev(ru.vector(s2.ndofs, 9))
        a, b = (integ.apply_add(u1, u2, torch.zeros(integ.ne, dtype=torch.float64, device="cuda")).cpu().numpy() for _ in range(2))
        assert np.array_equal(a, b) and a.min() > 0


@pytest.mark.parametrize("direction", ["grad", "curl"])
@pytest.mark.parametrize("p", [3, 4])
def test_flux_error_estimate(p, direction):
    """ComputeErrorEstimates (errorestimator.cpp:189-268) with the library's pieces at the orders the dense descriptors do not
    reach on hexahedra: smooth flux D = M^-1 Flux(eps) E by PCG + Jacobi on the sum-factorised mass of the smooth space (rel. tol
    1e-13), then eta_e^2 = int_e |eps^-1/2 D - eps^1/2 E|^2 -- "grad": E in H(curl), D in H(div) (GradFluxErrorEstimator); "curl":
    the other way round (CurlFluxErrorEstimator).  Against the same procedure through the oracle with a dense solve."""
    est, D, est_o, D_o, _ = _estimate(p, direction)
    eD, ee = _relerr(D, D_o), np.abs(est - est_o).max() / est_o.max()
    print(f"smooth flux {eD:.2e} estimates {ee:.2e}")
    assert eD < 1e-9 and ee < 1e-9
    assert est_o.min() > 0


def estimator_materials(mats=None):
    """(C, C^1/2, C^-1/2) as oracle contexts for the symmetric positive definite material of every attribute (default: one
    anisotropic tensor on both)."""
    mats = [np.array([[2.0, 0.3, 0.0], [0.3, 1.5, 0.1], [0.0, 0.1, 1.2]])] if mats is None else mats
    attr_mat = [0, 0] if len(mats) == 1 else [0, 1]
    sq, isq = [], []
    for m in mats:
        w, V = np.linalg.eigh(m)
        sq.append((V * np.sqrt(w)) @ V.T)
        isq.append((V / np.sqrt(w)) @ V.T)
    return tuple(po.CoeffCtx(attr_mat=attr_mat, mat_coeff=list(c)) for c in (mats, sq, isq))


def device_estimate(mesh, p, direction, field, mats=None):
    """The estimator procedure through the Python mirror on `mesh` at order p with p + 1 points per direction: returns
    (estimates, smooth flux, PCG iterations)."""
    import torch

    from palace_amd import ceed, linalg
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace

    nd, sp = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p)
    rhs_sp, smooth = (nd, sp) if direction == "grad" else (sp, nd)
    c_mat, c_sq, c_isq = estimator_materials(mats)
    geom = ceed.GeomFactorData(mesh, p + 1)
    ctx = linalg.Context()
    flux = ceed.mixedmass_operator(geom, rhs_sp, smooth, c_mat.pack())
    mass = (ceed.rtmass_operator if direction == "grad" else ceed.ndmass_operator)(geom, smooth, po.CoeffCtx().pack())
    M = linalg.ParOperator(ctx, mass, np.zeros(0, np.int32), linalg.DIAG_ONE)
    cg = linalg.cg(ctx, M, linalg.jacobi(ctx, M), rel_tol=1e-13, max_it=1000)
    qf = ceed.QF_HCURLHDIV_ERROR_33 if direction == "grad" else ceed.QF_HDIVHCURL_ERROR_33
    integ = ceed.HexElementErrorIntegrator(geom, rhs_sp, smooth, qf, np.concatenate([c_sq.pack(), c_isq.pack()]))
    Ed = _dev(field)
    rhs = torch.empty(smooth.ndofs, dtype=torch.float64, device="cuda")
    flux.mult(Ed, rhs)
    D = torch.zeros_like(rhs)
    cg.mult(rhs, D)
    assert cg.stats()["converged"]
    est = integ.apply_add(Ed, D, torch.zeros(integ.ne, dtype=torch.float64, device="cuda"))
    return est.cpu().numpy(), D.cpu().numpy(), cg.stats()["iterations"]


def _estimate(p, direction):
    kind, q1d = "ogrid15", p + 1
    (s1, o1), (s2, o2) = _sides(kind, p, q1d, direction == "grad")
    E = ru.vector(s1.ndofs, 3)
    est, D, its = device_estimate(_mesh(kind), p, direction, E)
    c_eps, c_sq, c_isq = estimator_materials()
    og = _ogeom(kind, q1d)
    Mo = po.CeedOperatorOracle(o2.lsize, o2.off, o2.sgn < 0, o2.interp, o2.interp, og,
                               po.QF_HDIV if direction == "grad" else po.QF_HCURL, po.CoeffCtx())
    qfo, qfe = ((po.QF_HCURLHDIV, po.QF_HCURLHDIV_ERROR) if direction == "grad" else (po.QF_HDIVHCURL, po.QF_HDIVHCURL_ERROR))
    rhs_o = po.MixedSpaceOracle(o1, o2, og, qfo, c_eps).apply_add(E, np.zeros(s2.ndofs))
    D_o = np.linalg.solve(Mo.assemble_sparse().toarray(), rhs_o)
    est_o = po.MixedSpaceOracle(o1, o2, og, qfe, c_sq, c_isq).error_add(E, D_o, np.zeros(o1.NE))
    return est, D, est_o, D_o, its


def test_refusals():
    import torch

    from palace_amd import ceed, lib
    from palace_amd.lib import PalaceAmdError

    kind, p, q1d = "ogrid15", 2, 3
    nd, sp = _spaces(kind, p)
    geom = _geom(kind, q1d)
    _, blob = util.make_ctx("aniso", 2)
    pair = np.concatenate([blob, blob])
    nd1, sp1 = _spaces(kind, 1)
    with pytest.raises(PalaceAmdError, match="same order"):
        ceed.Operator(sp1.ndofs, nd.ndofs).add_mixed_integrator(geom, nd, sp1, ceed.QF_HCURLHDIV_33, blob)
    with pytest.raises(PalaceAmdError, match="same order"):
        ceed.HexElementErrorIntegrator(geom, nd1, sp, ceed.QF_HCURLHDIV_ERROR_33, pair)
    nd4, sp4 = _spaces(kind, 4)
    with pytest.raises(PalaceAmdError, match=r"no H\(curl\) - H\(div\) hex kernel for order 4 with 4 points"):
        ceed.mixedmass_operator(_geom(kind, 4), nd4, sp4, blob)
    mesh = _mesh(kind)
    _, wts = po.hex_quadrature(q1d)
    dgeom = ceed.DenseGeomFactorData(mesh.elem_nodes, mesh.x, mesh.attr, po.mesh_q2_grad_table(q1d), wts)
    dgeom.q1d = q1d
    with pytest.raises(PalaceAmdError, match="pa_geom_create"):
        ceed.mixedmass_operator(dgeom, nd, sp, blob)
    with pytest.raises(PalaceAmdError, match="pa_geom_create"):
        ceed.HexElementErrorIntegrator(dgeom, nd, sp, ceed.QF_HCURLHDIV_ERROR_33, pair)
    with pytest.raises(PalaceAmdError, match="element types"):  # an H(curl) trial space needs the hcurlhdiv QFunction
        ceed.Operator(sp.ndofs, nd.ndofs).add_mixed_integrator(geom, nd, sp, ceed.QF_HDIVHCURL_33, blob)
    with pytest.raises(PalaceAmdError, match="element types"):
        ceed.HexElementErrorIntegrator(geom, sp, nd, ceed.QF_HCURLHDIV_ERROR_33, pair)
    with pytest.raises(PalaceAmdError, match="dimensions"):
        ceed.Operator(nd.ndofs, sp.ndofs).add_mixed_integrator(geom, nd, sp, ceed.QF_HCURLHDIV_33, blob)
    with pytest.raises(PalaceAmdError, match="mixed-space"):  # (a pair QFunction: no two-space form)
        ceed.Operator(sp.ndofs, nd.ndofs).add_mixed_integrator(geom, nd, sp, ceed.QF_HDIVMASS_33, blob)
    op = ceed.mixedmass_operator(geom, nd, sp, blob)
    with pytest.raises(PalaceAmdError, match="diagonal"):
        op.assemble_diagonal(torch.empty(sp.ndofs, dtype=torch.float64, device="cuda"))
    L = lib.load()
    assert not op.streams() and not op.supports_split() and L.pa_op_complex_fused(op.handle, op.handle) == 0
    assert L.pa_op_num_sub(op.handle) == 1 and L.pa_op_height(op.handle) == sp.ndofs and L.pa_op_width(op.handle) == nd.ndofs
    op.set_essential(np.arange(4, dtype=np.int32))
    avail = C.c_int(-1)
    lib.check(L.pa_op_prepare_fused_step(op.handle, C.byref(avail)))
    assert avail.value == 0
    x, y = _dev(ru.vector(nd.ndofs, 1)), torch.empty(sp.ndofs, dtype=torch.float64, device="cuda")
    with pytest.raises(PalaceAmdError, match="essential-dof form"):
        lib.check(L.pa_op_mult_essential(op.handle, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), None))


def test_full_assemble():
    """The rectangular matrix of the two-space operator reproduces its apply."""
    kind, p, q1d = "ogrid15", 2, 3
    op = _mass_operator(kind, p, q1d, True)
    A = op.full_assemble()
    x, _ = _mass_reference(kind, p, q1d, True, "nonsym")
    assert A.shape == (op.height, op.width) and _relerr(A @ x, _mult(op, x)) < 1e-12
