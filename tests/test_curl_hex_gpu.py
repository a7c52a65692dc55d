"""The sum-factorised discrete curl ND(p) -> RT(p) on hexahedra (palace_amd/csrc/pa_curl_hex.hip behind linalg.Curl /
pa_curl_create) and its transpose: against po.InterpOracle with rthex.hex_curl_matrix, against the dense interpolator of the
same matrix where that one exists (p <= 3), the exact sequence with the device gradient, and two identities that do not use the
element matrix at all.  On the two meshes of tests/rthex_util.py whose elements are handed over in seeded rotations (negative
orientation signs on both sides; 15 elements leave a partial wave or block at every order).  tests/test_curl_hex_host.py checks
the order list below against the compiled instantiations and the oracle-side facts on the CPU."""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import curl_util as cu
from tests import rthex_util as ru
from tests import transfer_util as tu

pytestmark = pytest.mark.gpu

CURL_ORDERS = [1, 2, 3, 4, 5]
REL = 1e-13   # transfers against the oracle, 2-norm (test_hex_transfer_gpu.py); rows here are sums of at most 12 products
ADJ = 1e-12   # adjointness (the same tests)
_ctx = []


def _context():
    from palace_amd import linalg

    if not _ctx:
        _ctx.append(linalg.Context())
    return _ctx[0]


def _curl(nd, rt, **kw):
    from palace_amd import linalg

    return linalg.Curl(_context(), nd, rt, **kw)


def _dense(nd, rt, p):
    from palace_amd import linalg

    dom = dict(offsets=nd.elem_dof_lex, lsize=nd.ndofs, orients=nd.elem_sign_lex < 0)
    return linalg.DenseInterp(_context(), dom, rt.restriction(interp_range=True), cu.matrix(p))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    import torch

    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("mesh_kind", ru.MESHES)
@pytest.mark.parametrize("p", CURL_ORDERS)
def test_curl_parity(mesh_kind, p):
    """Forward and transpose against the oracle into NaN-filled outputs, adjointness and repeatability of the device results."""
    import torch

    nd, rt = cu.spaces(mesh_kind, p)
    assert (nd.elem_sign_lex < 0).any() and (rt.elem_sign_lex < 0).any()
    T, o = _curl(nd, rt), cu.oracle(mesh_kind, p)
    xc, xf = cu.vectors(mesh_kind, p)
    yf_d = T.mult(_dev(xc), _nan(o.nf))
    yc_d = T.mult_transpose(_dev(xf), _nan(o.nc))
    yf, yc = yf_d.cpu().numpy(), yc_d.cpu().numpy()
    assert not np.isnan(yf).any() and not np.isnan(yc).any()  # the owner-copy store writes every range dof
    e_f, e_c = tu.rel(yf, o.mult(xc)), tu.rel(yc, o.mult_transpose(xf))
    adj = abs(xf @ yf - xc @ yc) / abs(xf @ yf)
    print(f"forward {e_f:.2e} transpose {e_c:.2e} adjointness {adj:.2e}")
    assert e_f < REL
    assert e_c < REL
    assert adj < ADJ
    assert torch.equal(T.mult(_dev(xc), _nan(o.nf)), yf_d)
    assert torch.equal(T.mult_transpose(_dev(xf), _nan(o.nc)), yc_d)


@pytest.mark.parametrize("mesh_kind", ru.MESHES)
@pytest.mark.parametrize("p", [1, 2, 3])
def test_curl_agrees_with_the_dense_interpolator(mesh_kind, p):
    nd, rt = cu.spaces(mesh_kind, p)
    T, Dn = _curl(nd, rt), _dense(nd, rt, p)
    xc, xf = cu.vectors(mesh_kind, p)
    for name, a, b in (("forward", T.mult(_dev(xc), _nan(rt.ndofs)), Dn.mult(_dev(xc), _nan(rt.ndofs))),
                       ("transpose", T.mult_transpose(_dev(xf), _nan(nd.ndofs)), Dn.mult_transpose(_dev(xf), _nan(nd.ndofs)))):
        e = tu.rel(a.cpu().numpy(), b.cpu().numpy())
        print(f"{name}: tensor against dense {e:.2e}")
        assert e < REL


def test_order_four_has_no_dense_curl():
    """An order-4 Nedelec hexahedron has 300 dofs, the dense interpolator stops at 256: why the tensor form exists."""
    from palace_amd.lib import PalaceAmdError

    nd, rt = cu.spaces("ogrid15", 4)
    assert nd.P == 300
    with pytest.raises(PalaceAmdError, match="element too large for the dense interpolator"):
        _dense(nd, rt, 4)


@pytest.mark.parametrize("p", CURL_ORDERS)
def test_exact_sequence_on_the_device(p):
    """C (G phi) with the device gradient and the device curl; the bound is cu.exactness_bound (the oracle alone stays within
    1.4 of its 16 units, tests/test_curl_hex_host.py)."""
    from palace_amd import linalg

    k = "ogrid15"
    h1 = tu.space(k, "h1", p)
    nd, rt = cu.spaces(k, p)
    G, T = linalg.Gradient(_context(), h1, nd), _curl(nd, rt)
    g = G.mult(_dev(ru.vector(h1.ndofs, 11 + p)), _nan(nd.ndofs))
    cg = T.mult(g, _nan(rt.ndofs)).cpu().numpy()
    g = g.cpu().numpy()
    bound = cu.exactness_bound(p, g)
    print(f"max |C G phi| = {np.abs(cg).max():.2e}, bound {bound:.2e}")
    assert np.linalg.norm(g) > 0 and not np.isnan(cg).any()
    assert np.abs(cg).max() <= bound


@pytest.mark.parametrize("mesh_kind", ru.MESHES)
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_basis_invariant_identities(mesh_kind, p):
    """(K a, a) = (M_RT C a, C a) with the sum-factorised curl-curl operator and Raviart-Thomas mass, and div-div of a discrete
    curl vanishes: neither uses rthex.hex_curl_matrix.  Tolerances of test_rt_hex_gpu.py::test_rt_hex_structure."""
    import torch

    from palace_amd import ceed
    from tests.test_rt_hex_gpu import _geom, _operator

    q1d = p + 1
    nd, rt = cu.spaces(mesh_kind, p)
    geom = _geom(mesh_kind, q1d)
    a = _dev(ru.vector(nd.ndofs, p))
    b = _curl(nd, rt).mult(a, _nan(rt.ndofs))
    K = ceed.curlcurl_operator(geom, nd, ceed.coefficient_context(3))
    M1 = ceed.rtmass_operator(geom, rt, ceed.coefficient_context(3))
    ka, mb = torch.empty_like(a), torch.empty_like(b)
    K.mult(a, ka)
    M1.mult(b, mb)
    e_k, e_m = float(a @ ka), float(b @ mb)
    print(f"(K a, a) = {e_k:.15e}, (M C a, C a) = {e_m:.15e}, difference {abs(e_k - e_m) / abs(e_k):.2e}")
    assert abs(e_k - e_m) < 1e-11 * abs(e_k)
    D = _operator(mesh_kind, p, q1d, "divdiv")
    dd, yd = torch.empty_like(b), torch.empty_like(b)
    D.assemble_diagonal(dd)
    D.mult(b, yd)
    print(f"max |D C a| = {float(yd.abs().max()):.2e}")
    assert float(yd.abs().max()) < 1e-11 * float(b.abs().max()) * float(dd.abs().max())


def test_many_blocks_and_the_four_dof_gather():
    """3 520 elements at order 3 (220 blocks); the transposed gather takes four dofs per thread (k_gather_t<4>) from 2^18 domain
    dofs on: 294 129 Nedelec dofs, the last block of 1 024 partial."""
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.fem.mesh import cylinder_for_dofs

    mesh = cylinder_for_dofs(2.75e5, 3)
    nd, rt = NDHexSpace(mesh, 3), rthex.RTHexSpace(mesh, 3)
    assert mesh.ne == 3520 and nd.ndofs == 294129 and nd.ndofs >= 1 << 18 and nd.ndofs % 1024 != 0
    o, T = cu.oracle_of(nd, rt, 3), _curl(nd, rt)
    rng = np.random.default_rng(35)
    xc, xf = rng.uniform(-1, 1, nd.ndofs), rng.uniform(-1, 1, rt.ndofs)
    yc = T.mult_transpose(_dev(xf), _nan(nd.ndofs)).cpu().numpy()
    yf = T.mult(_dev(xc), _nan(rt.ndofs)).cpu().numpy()
    assert not np.isnan(yc).any() and not np.isnan(yf).any()
    e_c, e_f = tu.rel(yc, o.mult_transpose(xf)), tu.rel(yf, o.mult(xc))
    print(f"transpose {e_c:.2e} forward {e_f:.2e}")
    assert e_c < REL
    assert e_f < REL


def test_staging_branch_without_a_halo():
    """Fewer true than local Raviart-Thomas dofs on one rank (no halo): the operator runs on its staging vectors.  mult gives the
    first n_true entries of the full operator's result and mult_transpose what the full one gives for the zero-padded input."""
    import torch

    p = 3
    nd, rt = cu.spaces("ogrid15", p)
    nt = rt.ndofs - 37
    full, part = _curl(nd, rt), _curl(nd, rt, n_true_rt=nt)
    xc, xf = cu.vectors("ogrid15", p)
    yf = full.mult(_dev(xc), _nan(rt.ndofs))
    for _ in range(2):  # (the second call finds the staging vectors used)
        assert torch.equal(part.mult(_dev(xc), _nan(nt)), yf[:nt])
    xp = xf.copy()
    xp[nt:] = 0.0
    yc = full.mult_transpose(_dev(xp), _nan(nd.ndofs))
    assert not torch.isnan(yc).any() and not torch.isnan(yf).any()
    for _ in range(2):
        assert torch.equal(part.mult_transpose(_dev(xf[:nt]), _nan(nd.ndofs)), yc)
    assert tu.rel(yc.cpu().numpy(), cu.oracle("ogrid15", p).mult_transpose(xp)) < REL


def _raw_create(nd, rt, edit):
    """pa_curl_create on the descriptors of (nd, rt) after `edit(rn, bn, rr, br, keep)` changed them."""
    from palace_amd import lib as _lib
    from palace_amd.ceed import _basis_desc, _ptr, _restriction_desc

    p = rt.p
    Dg = cu.derivative_1d(p)
    rn, k1 = _restriction_desc(nd)
    rr, k2 = _restriction_desc(rt)
    bn, k3 = _basis_desc(nd, p + 1)
    br, k4 = _basis_desc(rt, p + 1)
    keep = []
    edit(rn, bn, rr, br, keep)
    h = C.c_void_p()
    _lib.check(_lib.load().pa_curl_create(_context().handle, C.byref(rn), C.byref(bn), C.byref(rr), C.byref(br), _ptr(Dg), None,
                                          nd.ndofs, rt.ndofs, C.byref(h)))
    _lib.load().pa_interp_destroy(h)


def test_refusals():
    from palace_amd.ceed import _ptr
    from palace_amd.lib import PalaceAmdError

    nd, rt = cu.spaces("ogrid15", 2)
    h1 = tu.space("ogrid15", "h1", 2)
    with pytest.raises(PalaceAmdError, match="maps a Nedelec space to a Raviart-Thomas space"):
        _curl(h1, rt)
    with pytest.raises(PalaceAmdError, match="maps a Nedelec space to a Raviart-Thomas space"):
        _curl(nd, nd)
    with pytest.raises(PalaceAmdError, match="same order on both sides"):
        _curl(tu.space("ogrid15", "nd", 3), rt)
    with pytest.raises(PalaceAmdError, match="order above 5"):
        _curl(tu.space("ogrid15", "nd", 6), ru.space("ogrid15", 6))
    with pytest.raises(PalaceAmdError, match="same elements on both sides"):
        _curl(tu.space("cyl80", "nd", 2), rt)
    short = copy.copy(rt)
    short.P = rt.P - 1
    with pytest.raises(PalaceAmdError, match="restriction sizes do not match the bases"):
        _curl(nd, short)
    for side in (0, 2):  # curl_orients on the Nedelec side, on the Raviart-Thomas side
        def edit(*descs, side=side):
            r, keep = descs[side], descs[4]
            keep.append(np.zeros((r.num_elem, r.elem_size, 3), dtype=np.int8))
            r.curl_orients = _ptr(keep[-1])

        with pytest.raises(PalaceAmdError, match="sign orientations, not curl_orients"):
            _raw_create(nd, rt, edit)
    with pytest.raises(PalaceAmdError, match="true dof counts exceed local sizes"):
        _curl(nd, rt, n_true_rt=rt.ndofs + 1)
    with pytest.raises(PalaceAmdError, match="true dof counts exceed local sizes"):
        _curl(nd, rt, n_true_nd=nd.ndofs + 1)
    with pytest.raises(PalaceAmdError, match="ghost dofs on the Nedelec side need a halo plan"):
        _curl(nd, rt, n_true_nd=nd.ndofs - 1)
    _raw_create(nd, rt, lambda *descs: None)  # (the unedited descriptors are accepted)
