"""Sum-factorised Raviart-Thomas hexahedra (palace_amd/csrc/pa_rt_hex.hip through pa_op_add_sub with PA_FE_HDIV): the H(div)
mass, div-div and div-div + mass operators against the oracle and against the dense-table path, on meshes whose elements are
handed over in every rotation (tests/rthex_util.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import util

pytestmark = pytest.mark.gpu
REL = 1e-12

PQ = [(1, 2), (2, 3), (3, 4), (4, 5), (1, 4), (2, 4), (3, 5), (1, 3), (1, 5), (2, 5)]  # PA_HEX_PQ_LIST
FORMS = ("mass", "divdiv", "divdivmass")
_geoms = {}


def _geom(kind, q1d):
    from palace_amd import ceed

    if (kind, q1d) not in _geoms:
        _geoms[kind, q1d] = ceed.GeomFactorData(ru.mesh(kind), q1d)
    return _geoms[kind, q1d]


def _operator(kind, p, q1d, form, mass="aniso", dense=None, **kw):
    from palace_amd import ceed

    sp, geom = ru.space(kind, p), _geom(kind, q1d)
    _, blob = util.make_ctx(mass, 2)
    if kw:  # another native order (the signed dof_map test)
        return ceed.Operator(sp.ndofs, sp.ndofs).add_integrator(geom, sp, ceed.QF_HDIV_33, blob, ceed.EVAL_INTERP, dense,
                                                                **kw).finalize()
    if form == "mass":
        return ceed.rtmass_operator(geom, sp, blob, dense)
    if form == "divdiv":
        return ceed.divdiv_operator(geom, sp, ru.div_ctx().pack(), dense)
    return ceed.divdivmass_operator(geom, sp, blob, ru.div_ctx().pack(), dense)


def _dense_operator(kind, p, q1d, mass="aniso"):
    """The dense-table path, as tests/test_rt_gpu.py::test_rt_hex_mass_and_discrete_curl builds it."""
    from palace_amd import ceed

    mesh, sp = ru.mesh(kind), ru.space(kind, p)
    _, wts = po.hex_quadrature(q1d)
    dgeom = ceed.DenseGeomFactorData(mesh.elem_nodes, mesh.x, mesh.attr, po.mesh_q2_grad_table(q1d), wts)
    rint, _ = ru.tables(p, q1d)
    _, blob = util.make_ctx(mass, 2)
    block = ceed.DenseBlock(ceed.FE_HDIV, sp.ndofs, sp.elem_dof_lex, rint, None, orients=sp.elem_sign_lex < 0)
    return ceed.Operator(sp.ndofs, sp.ndofs).add_dense_integrator(dgeom, block, ceed.QF_HDIV_33, blob, ceed.EVAL_INTERP).finalize()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mult(op, x):
    import torch

    y = torch.full((x.size,), 7.0, dtype=torch.float64, device="cuda")  # Mult overwrites
    op.mult(_dev(x), y)
    return y.cpu().numpy()


def _relerr(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("qdata", ["packed", "matrixfree"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("p,q1d", PQ)
def test_rt_hex_parity(monkeypatch, p, q1d, form, qdata, kind):
    """mult, add_mult onto a non-zero y and assemble_diagonal against the oracle, for both D forms."""
    import torch

    if qdata == "matrixfree":
        monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    op = _operator(kind, p, q1d, form)
    x, ref = ru.oracle_mult(kind, p, q1d, form)
    assert op.is_symmetric()
    e = _relerr(_mult(op, x), ref)
    print(f"mult {e:.2e}")
    assert e < REL
    y0 = ru.vector(x.size, 5)
    y = _dev(y0)
    op.add_mult(_dev(x), y)
    e = np.abs(y.cpu().numpy() - (y0 + ref)).max() / np.abs(ref).max()
    print(f"add_mult {e:.2e}")
    assert e < REL
    d = torch.full((x.size,), 3.0, dtype=torch.float64, device="cuda")
    op.assemble_diagonal(d)
    e = _relerr(d.cpu().numpy(), ru.oracle_diag(kind, p, q1d, form))
    print(f"diagonal {e:.2e}")
    assert e < REL
    assert op.height == x.size and op.algorithmic_bytes() > 0


@pytest.mark.parametrize("form", FORMS)
def test_rt_hex_dense_tables_checked(form):
    """With the dense value / divergence tables passed the result is unchanged; a wrong table is refused."""
    from palace_amd.lib import PalaceAmdError

    kind, p, q1d = "ogrid15", 2, 3
    rint, rdiv = ru.tables(p, q1d)
    x, ref = ru.oracle_mult(kind, p, q1d, form)
    plain = _mult(_operator(kind, p, q1d, form), x)
    checked = _mult(_operator(kind, p, q1d, form, dense=(rint, rdiv)), x)
    assert np.array_equal(plain, checked) and _relerr(checked, ref) < REL
    bad_v, bad_d = rint.copy(), rdiv.copy()
    bad_v[1, 5, 7] += 1e-3
    bad_d[4, 9] += 1e-3
    for dense in ((bad_v, rdiv), (rint, bad_d)):
        with pytest.raises(PalaceAmdError, match="dense basis table"):
            _operator(kind, p, q1d, form, dense=dense)


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("form", ["mass", "divdivmass"])
@pytest.mark.parametrize("p,q1d", [(1, 2), (2, 3), (3, 4), (4, 5)])
def test_rt_hex_nonsymmetric_material(p, q1d, form, kind):
    """A general 3 x 3 material: the matrix-free D; A^T through the transposed matrices."""
    import torch

    op = _operator(kind, p, q1d, form, mass="nonsym")
    x, ref = ru.oracle_mult(kind, p, q1d, form, mass="nonsym")
    assert not op.is_symmetric()
    ax = _mult(op, x)
    assert _relerr(ax, ref) < REL
    z = ru.vector(x.size, 17)
    atz = torch.empty(x.size, dtype=torch.float64, device="cuda")
    op.mult_transpose(_dev(z), atz)
    atz = atz.cpu().numpy()
    lhs, rhs = z @ ax, atz @ x
    print(f"transpose identity {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)
    assert np.abs(atz - ax).max() > 1e-6 * np.abs(ax).max()  # A^T really differs from A
    # ... and A^T is the oracle's operator with every material matrix transposed
    _, tref = ru.oracle_mult(kind, p, q1d, form, mass="nonsym_t", x=z)
    assert _relerr(atz, tref) < REL
    # the diagonal of a non-symmetric material (matrix-free D)
    d = torch.full((x.size,), 3.0, dtype=torch.float64, device="cuda")
    op.assemble_diagonal(d)
    assert _relerr(d.cpu().numpy(), ru.oracle_diag(kind, p, q1d, form, mass="nonsym")) < REL


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("p", [2, 3])
def test_rt_hex_same_numbers_as_dense_path(p, kind):
    q1d = p + 1
    x, _ = ru.oracle_mult(kind, p, q1d, "mass")
    a, b = _mult(_operator(kind, p, q1d, "mass"), x), _mult(_dense_operator(kind, p, q1d), x)
    assert _relerr(a, b) < 1e-12


def test_rt_hex_signed_dof_map():
    """A seeded signed permutation of the local dofs as the native order: offsets permuted to match, orientation flags XORed
    with the map's signs -- the same operator.  A map that is no permutation is refused."""
    from palace_amd.lib import PalaceAmdError

    kind, p, q1d = "ogrid15", 3, 4
    sp = ru.space(kind, p)
    rng = np.random.default_rng(3)
    nat = rng.permutation(sp.P)
    flip = rng.integers(0, 2, sp.P).astype(bool)
    dof_map = np.where(flip, -1 - nat, nat).astype(np.int32)
    ori = np.empty(sp.elem_dof_lex.shape, dtype=np.uint8)  # (the offsets are permuted to match by add_integrator)
    ori[:, nat] = (sp.elem_sign_lex < 0) ^ flip[None, :]
    assert flip.any() and not flip.all()
    x, _ = ru.oracle_mult(kind, p, q1d, "mass")
    lex = _mult(_operator(kind, p, q1d, "mass"), x)
    got = _mult(_operator(kind, p, q1d, "mass", dof_map=dof_map, orients=ori), x)
    assert _relerr(got, lex) < 1e-12
    bad = dof_map.copy()
    bad[1] = bad[0]
    with pytest.raises(PalaceAmdError, match="signed permutation"):
        _operator(kind, p, q1d, "mass", dof_map=bad, orients=ori)


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("p", [1, 2, 3])
def test_rt_hex_structure(p, kind):
    """(K a, a) = (M_RT C a, C a) with the sum-factorised curl-curl operator, the dense interpolator of the discrete curl and
    the new mass; div-div of a discrete curl vanishes."""
    import torch

    from palace_amd import ceed, linalg
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace

    q1d = p + 1
    mesh, sp, geom = ru.mesh(kind), ru.space(kind, p), _geom(kind, q1d)
    nd = NDHexSpace(mesh, p)
    ctx = linalg.Context()
    dom = dict(offsets=nd.elem_dof_lex, lsize=nd.ndofs, orients=nd.elem_sign_lex < 0)
    Cd = linalg.DenseInterp(ctx, dom, sp.restriction(interp_range=True), rthex.hex_curl_matrix(p))
    a = _dev(ru.vector(nd.ndofs, p))
    b = torch.empty(sp.ndofs, dtype=torch.float64, device="cuda")
    Cd.mult(a, b)
    K = ceed.curlcurl_operator(geom, nd, ceed.coefficient_context(3))
    M1 = ceed.rtmass_operator(geom, sp, ceed.coefficient_context(3))
    ka, mb = torch.empty_like(a), torch.empty_like(b)
    K.mult(a, ka)
    M1.mult(b, mb)
    e_k, e_m = float(a @ ka), float(b @ mb)
    assert abs(e_k - e_m) < 1e-11 * abs(e_k)
    D = _operator(kind, p, q1d, "divdiv")
    dd, yd = torch.empty_like(b), torch.empty_like(b)
    D.assemble_diagonal(dd)
    D.mult(b, yd)
    assert float(yd.abs().max()) < 1e-11 * float(b.abs().max()) * float(dd.abs().max())


@pytest.mark.parametrize("form", FORMS)
def test_rt_hex_full_assemble(form):
    kind, p, q1d = "ogrid15", 2, 3
    op = _operator(kind, p, q1d, form)
    A = op.full_assemble()
    x, _ = ru.oracle_mult(kind, p, q1d, form)
    ax = _mult(op, x)
    assert _relerr(A @ x, ax) < 1e-12
    assert abs(A - A.T).max() < 1e-12 * abs(A).max()


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("policy", ["one", "zero"])
@pytest.mark.parametrize("qdata", ["packed", "matrixfree"])
def test_rt_hex_essential_dofs(monkeypatch, qdata, policy, kind):
    """ParOperator with the boundary-face dofs essential: entries read as zero, rows fixed."""
    import torch

    from palace_amd import linalg

    if qdata == "matrixfree":
        monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    p, q1d, form = 2, 3, "divdivmass"
    op = _operator(kind, p, q1d, form)
    ess = ru.boundary_dofs(kind, p)
    assert 0 < ess.size < op.height
    ctx = linalg.Context()
    A = linalg.ParOperator(ctx, op, ess, linalg.DIAG_ONE if policy == "one" else linalg.DIAG_ZERO)
    x = ru.vector(op.height, 23)
    tx = x.copy()
    tx[ess] = 0.0
    orc = ru.oracle(kind, p, q1d, form)
    ref = orc.apply_add(tx, np.zeros(x.size))
    scale = np.abs(ref).max()
    ref[ess] = x[ess] if policy == "one" else 0.0
    y = torch.full((x.size,), 7.0, dtype=torch.float64, device="cuda")
    A.mult(_dev(x), y)
    assert np.abs(y.cpu().numpy() - ref).max() < REL * scale
    # the C entry point itself: the single block fixes the essential rows in its gather
    from palace_amd import lib

    handled = C.c_int(-1)
    y2 = torch.full((x.size,), 7.0, dtype=torch.float64, device="cuda")
    xd = _dev(x)
    lib.check(lib.load().pa_op_mult_essential_diag(op.handle, C.c_void_p(xd.data_ptr()), C.c_void_p(y2.data_ptr()),
                                                   C.c_int(1 if policy == "one" else 0), None, C.byref(handled)))
    torch.cuda.synchronize()
    assert handled.value == 1 and np.abs(y2.cpu().numpy() - ref).max() < REL * scale
    d = torch.empty_like(y)
    A.assemble_diagonal(d)
    dref = ru.oracle_diag(kind, p, q1d, form).copy()
    dref[ess] = 1.0 if policy == "one" else 0.0
    assert np.abs(d.cpu().numpy() - dref).max() < REL * np.abs(dref).max()


@pytest.mark.parametrize("kind,p", [("cyl80", 3), ("ogrid15", 2)])
def test_rt_hex_mass_solve(kind, p):
    """The solve the kernel exists for: PCG + Jacobi on the RT mass recovers d0 from b = M d0; the iteration count is that of
    the same solve on the dense-path operator (+-1)."""
    import torch

    from palace_amd import linalg

    q1d = p + 1
    ctx = linalg.Context()
    its = []
    d0 = ru.vector(ru.space(kind, p).ndofs, 31)
    for op in (_operator(kind, p, q1d, "mass"), _dense_operator(kind, p, q1d)):
        M = linalg.ParOperator(ctx, op, np.zeros(0, dtype=np.int32))
        b, d = torch.empty(d0.size, dtype=torch.float64, device="cuda"), torch.zeros(d0.size, dtype=torch.float64, device="cuda")
        M.mult(_dev(d0), b)
        solver = linalg.cg(ctx, M, linalg.jacobi(ctx, M), rel_tol=1e-12, max_it=1000)
        solver.mult(b, d)
        st = solver.stats()
        assert st["converged"]
        assert np.linalg.norm(d.cpu().numpy() - d0) < 1e-9 * np.linalg.norm(d0)
        its.append(st["iterations"])
    print("iterations (tensor, dense):", its)
    assert abs(its[0] - its[1]) <= 1


def test_rt_hex_refusals_and_capabilities():
    from palace_amd import ceed, lib
    from palace_amd.fem import rthex
    from palace_amd.lib import PalaceAmdError

    kind = "ogrid15"
    mesh = ru.mesh(kind)
    _, blob = util.make_ctx("aniso", 2)
    sp4 = rthex.RTHexSpace(mesh, 4)
    with pytest.raises(PalaceAmdError, match=r"no H\(div\) hex kernel for order 4 with 4 points"):
        ceed.rtmass_operator(_geom(kind, 4), sp4, blob)
    sp, geom = ru.space(kind, 2), _geom(kind, 3)
    supported = r"PA_QF_HDIV_33.*PA_QF_L2_1.*PA_QF_L2MASS_33"
    with pytest.raises(PalaceAmdError, match=supported):
        ceed.Operator(sp.ndofs, sp.ndofs).add_integrator(geom, sp, ceed.QF_HCURL_33, blob, ceed.EVAL_INTERP)
    with pytest.raises(PalaceAmdError, match=supported):
        ceed.Operator(sp.ndofs, sp.ndofs).add_integrator(geom, sp, ceed.QF_L2_1, ru.div_ctx().pack(), ceed.EVAL_INTERP)
    op = _operator(kind, 2, 3, "mass")
    with pytest.raises(PalaceAmdError, match=r"H\(curl\) and H1"):
        op.coarsen(geom, ru.space(kind, 1))
    with pytest.raises(PalaceAmdError, match=r"H\(curl\)"):
        ceed.Operator(sp.ndofs, sp.ndofs).add_integrator_sum(geom, sp, [(1.0, ceed.QF_HDIV_33, blob)])
    L = lib.load()
    assert not op.streams() and not op.supports_split()
    assert L.pa_op_complex_fused(op.handle, op.handle) == 0
    op.set_essential(ru.boundary_dofs(kind, 2))
    avail = C.c_int(-1)
    lib.check(L.pa_op_prepare_fused_step(op.handle, C.byref(avail)))
    assert avail.value == 0
    assert L.pa_op_num_sub(op.handle) == 1 and L.pa_op_height(op.handle) == sp.ndofs and L.pa_op_width(op.handle) == sp.ndofs
    # mult2 falls back to two applies
    import torch

    x0, x1 = ru.vector(sp.ndofs, 1), ru.vector(sp.ndofs, 2)
    y0 = torch.empty(sp.ndofs, dtype=torch.float64, device="cuda")
    y1 = torch.empty_like(y0)
    op.mult2(_dev(x0), _dev(x1), y0, y1)
    assert np.array_equal(y0.cpu().numpy(), _mult(op, x0)) and np.array_equal(y1.cpu().numpy(), _mult(op, x1))
    # the bytes the packed mass streams: six rows per point, the sorted index and its slot per entry
    Q, P, ne = 27, sp.P, mesh.ne
    assert op.algorithmic_bytes() == ne * (Q * 6 * 8 + P * 6) + 16.0 * sp.ndofs
