"""The p-prolongation between Raviart-Thomas spaces on tensor hexahedra (palace_amd/csrc/pa_prolong_rt_hex.hip) and its
transpose against po.InterpOracle for every compiled pair (six specialised instantiations, the generic form at fine order 5), on
the two meshes of tests/rthex_util.py whose elements are handed over in seeded rotations; the commuting diagram with the discrete
curl, the Galerkin identity P^T M_f P = M_c and the dense interpolator on the device; and a p-multigrid cycle over RT masses
through the Python mirror.  tests/test_rt_transfer_host.py checks the pair list against the compiled one and the oracle-side
facts on the CPU."""
import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import rt_transfer_util as rtu
from tests import rthex_util as ru
from tests import transfer_util as tu
from tests import util

pytestmark = pytest.mark.gpu

PAIRS = [(1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4), (1, 5), (2, 5), (3, 5), (4, 5)]
GALERKIN_PAIRS = [(pc, pf) for pc, pf in PAIRS if pf <= 4]  # (pc, pf + 1) is a compiled mass kernel (PA_HEX_PQ_LIST)

REL = 1e-13   # transfers against the oracle, 2-norm (test_hex_transfer_gpu.py)
ADJ = 1e-12   # adjointness (the same file)
_ctx = []
_geoms = {}


def _context():
    from palace_amd import linalg

    if not _ctx:
        _ctx.append(linalg.Context())
    return _ctx[0]


def _geom(kind, q1d):
    from palace_amd import ceed

    if (kind, q1d) not in _geoms:
        _geoms[kind, q1d] = ceed.GeomFactorData(ru.mesh(kind), q1d)
    return _geoms[kind, q1d]


def _interp(c, f, **kw):
    from palace_amd import linalg

    return linalg.Interp(_context(), c, f, **kw)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    import torch

    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("mesh_kind", ru.MESHES)
@pytest.mark.parametrize("pc,pf", PAIRS)
def test_rt_transfer_parity(mesh_kind, pc, pf):
    """Forward and transpose against the oracle into NaN-filled outputs, adjointness and repeatability of the device results."""
    import torch

    c, f = rtu.spaces(mesh_kind, pc, pf)
    assert (c.elem_sign_lex < 0).any() and (f.elem_sign_lex < 0).any()
    T, o = _interp(c, f), rtu.oracle(mesh_kind, pc, pf)
    xc, xf = rtu.vectors(mesh_kind, pc, pf)
    yf_d = T.mult(_dev(xc), _nan(o.nf))
    yc_d = T.mult_transpose(_dev(xf), _nan(o.nc))
    yf, yc = yf_d.cpu().numpy(), yc_d.cpu().numpy()
    assert not np.isnan(yf).any() and not np.isnan(yc).any()  # the owner-copy store writes every fine dof
    e_f, e_c = tu.rel(yf, o.mult(xc)), tu.rel(yc, o.mult_transpose(xf))
    adj = abs(xf @ yf - xc @ yc) / abs(xf @ yf)
    print(f"forward {e_f:.2e} transpose {e_c:.2e} adjointness {adj:.2e}")
    assert e_f < REL
    assert e_c < REL
    assert adj < ADJ
    assert torch.equal(T.mult(_dev(xc), _nan(o.nf)), yf_d)
    assert torch.equal(T.mult_transpose(_dev(xf), _nan(o.nc)), yc_d)


@pytest.mark.parametrize("pc,pf", PAIRS)
def test_commutes_with_the_curl_on_the_device(pc, pf):
    """Curl_f P_nd a = P_rt Curl_c a: four device operators, no oracle."""
    from palace_amd import linalg

    k = "ogrid15"
    nc, nf, rc, rf = tu.space(k, "nd", pc), tu.space(k, "nd", pf), ru.space(k, pc), ru.space(k, pf)
    P_nd, P_rt = _interp(nc, nf), _interp(rc, rf)
    C_c, C_f = linalg.Curl(_context(), nc, rc), linalg.Curl(_context(), nf, rf)
    x = _dev(ru.vector(nc.ndofs, 9 + 10 * pc + pf))
    a = C_f.mult(P_nd.mult(x, _nan(nf.ndofs)), _nan(rf.ndofs)).cpu().numpy()
    b = P_rt.mult(C_c.mult(x, _nan(rc.ndofs)), _nan(rf.ndofs)).cpu().numpy()
    err = tu.rel(a, b)
    print(f"commuting diagram {err:.2e}")
    assert np.linalg.norm(b) > 0.0 and err < 1e-12


@pytest.mark.parametrize("mesh_kind", ru.MESHES)
@pytest.mark.parametrize("pc,pf", GALERKIN_PAIRS)
def test_galerkin_operator_on_the_device(mesh_kind, pc, pf):
    """P^T M_f P x against the mass of order pc on the rule of order pf (two materials, anisotropic coefficient)."""
    from palace_amd import ceed

    c, f = rtu.spaces(mesh_kind, pc, pf)
    _, blob = util.make_ctx("aniso", 2)
    geom = _geom(mesh_kind, pf + 1)
    Mf, Mc = ceed.rtmass_operator(geom, f, blob), ceed.rtmass_operator(geom, c, blob)
    P = _interp(c, f)
    x = _dev(ru.vector(c.ndofs, 11 + 10 * pc + pf))
    a = P.mult_transpose(Mf.mult(P.mult(x, _nan(f.ndofs)), _nan(f.ndofs)), _nan(c.ndofs)).cpu().numpy()
    b = Mc.mult(x, _nan(c.ndofs)).cpu().numpy()
    err = tu.rel(a, b)
    print(f"Galerkin {err:.2e}")
    assert not np.isnan(b).any() and err < 1e-12


@pytest.mark.parametrize("pc,pf", GALERKIN_PAIRS)
def test_same_numbers_as_the_dense_interpolator(pc, pf):
    """linalg.DenseInterp with the element matrix of tests/rt_transfer_util.py (240 dofs per element at order 4 fit)."""
    from palace_amd import linalg

    k = "ogrid15"
    c, f = rtu.spaces(k, pc, pf)
    D = linalg.DenseInterp(_context(), c.restriction(), f.restriction(), rtu.matrix(pc, pf))
    T = _interp(c, f)
    xc, xf = rtu.vectors(k, pc, pf)
    e_f = tu.rel(T.mult(_dev(xc), _nan(f.ndofs)).cpu().numpy(), D.mult(_dev(xc), _nan(f.ndofs)).cpu().numpy())
    e_c = tu.rel(T.mult_transpose(_dev(xf), _nan(c.ndofs)).cpu().numpy(), D.mult_transpose(_dev(xf), _nan(c.ndofs)).cpu().numpy())
    print(f"forward {e_f:.2e} transpose {e_c:.2e}")
    assert e_f < 1e-13
    assert e_c < 1e-13


@pytest.mark.parametrize("pc,pf", [(2, 3), (1, 5)])
def test_staging_branch_without_a_halo(pc, pf):
    """Fewer true than local fine dofs on one rank (no halo): the operator runs on its staging vectors.  mult gives the first
    n_true entries of the full operator's result and mult_transpose what the full one gives for the zero-padded input."""
    import torch

    k = "ogrid15"
    c, f = rtu.spaces(k, pc, pf)
    nt = f.ndofs - 37
    full, part = _interp(c, f), _interp(c, f, n_true_f=nt)
    xc, xf = rtu.vectors(k, pc, pf)
    yf = full.mult(_dev(xc), _nan(f.ndofs))
    for _ in range(2):  # (the second call finds the staging vectors used)
        assert torch.equal(part.mult(_dev(xc), _nan(nt)), yf[:nt])
    xp = xf.copy()
    xp[nt:] = 0.0
    yc = full.mult_transpose(_dev(xp), _nan(c.ndofs))
    assert not torch.isnan(yc).any() and not torch.isnan(yf).any()
    for _ in range(2):
        assert torch.equal(part.mult_transpose(_dev(xf[:nt]), _nan(c.ndofs)), yc)
    assert tu.rel(yc.cpu().numpy(), rtu.oracle(k, pc, pf).mult_transpose(xp)) < REL


def test_refusals():
    from palace_amd.fem import rthex
    from palace_amd.lib import PalaceAmdError

    k = "ogrid15"
    with pytest.raises(PalaceAmdError, match="same element family"):
        _interp(tu.space(k, "nd", 1), ru.space(k, 2))
    with pytest.raises(PalaceAmdError, match="same element family"):
        _interp(ru.space(k, 1), tu.space(k, "nd", 2))
    for pc, pf in ((2, 2), (3, 2)):
        with pytest.raises(PalaceAmdError, match="unsupported orders for prolongation"):
            _interp(ru.space(k, pc), ru.space(k, pf))
    with pytest.raises(PalaceAmdError, match="unsupported orders for prolongation"):
        _interp(ru.space(k, 2), rthex.RTHexSpace(ru.mesh(k), 6))


def test_multigrid_over_rt_masses():
    """linalg.gmg over the unit-coefficient RT masses of orders 1, 2, 3 on ogrid15, every level assembled on the four-point rule,
    configured as the flux projector's (4th-kind Chebyshev order 2, one pre and one post step): one cycle against po.GMGOracle
    with the device's lambda_max per level and the coarse Jacobi-PCG restated, then PCG iteration counts against the oracle
    and against Jacobi."""
    import torch

    from palace_amd import ceed, linalg

    k, levels, q1d = "ogrid15", [1, 2, 3], 4
    ctx = _context()
    sp = [ru.space(k, p) for p in levels]
    _, blob = util.make_ctx("identity")
    none = np.zeros(0, dtype=np.int32)
    ops = [ceed.rtmass_operator(_geom(k, q1d), s, blob) for s in sp]
    A = [linalg.ParOperator(ctx, op, none) for op in ops]
    P = [_interp(sp[l], sp[l + 1]) for l in range(2)]
    ctol = 1e-10  # (one coarse iteration more or less moves the cycle by ~1e-10, below the bound of the comparison)
    coarse = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=ctol, max_it=200)
    B = linalg.gmg(ctx, A, P, coarse, cheby_order=2)
    lam = [linalg.chebyshev(ctx, A[l], order=2).lambda_max() for l in (1, 2)]
    oA = [rtu.SparseLevel(rtu.mass_oracle(k, p, q1d, "unit")) for p in levels]
    d0 = 1.0 / oA[0].diagonal()
    oB = rtu.gmg_oracle(oA, [rtu.oracle(k, 1, 2), rtu.oracle(k, 2, 3)], lam,
                        lambda r: po.pcg(oA[0].mult, r, lambda v: d0 * v, rel_tol=ctol, max_it=200)[0])
    n = sp[-1].ndofs
    new = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")  # noqa: E731
    r = ru.vector(n, 8)
    e_cycle = tu.rel(B.mult(_dev(r), new()).cpu().numpy(), oB.mult(r))
    print(f"one cycle {e_cycle:.2e}")
    assert e_cycle < 1e-8
    b = oA[-1].mult(ru.vector(n, 77))
    K = linalg.cg(ctx, A[-1], B, rel_tol=1e-8, max_it=200)
    x = K.mult(_dev(b), new()).cpu().numpy()
    xo, it, _ = po.pcg(oA[-1].mult, b, oB.mult, rel_tol=1e-8, max_it=200)
    st = K.stats()
    KJ = linalg.cg(ctx, A[-1], linalg.jacobi(ctx, A[-1]), rel_tol=1e-8, max_it=200)
    KJ.mult(_dev(b), new())
    it_j = KJ.stats()["iterations"]
    print(f"PCG iterations: multigrid {st['iterations']} (oracle {it}), Jacobi {it_j}")
    assert st["converged"] and abs(st["iterations"] - it) <= 1, (st, it)
    assert tu.rel(x, xo) < 1e-6
    assert KJ.stats()["converged"] and st["iterations"] < it_j
