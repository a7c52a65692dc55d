"""The conforming prolongation with hanging-entity constraints (palace_amd/csrc/pa_conform.hip: k_conform_prolongate and
k_conform_restrict, one launch each, here in their one-vector form) against scipy: lx = P x and y = P^T ly with P = [I; C],
masked and unmasked, overwrite and add, the |C|^T form of the diagonal and both essential-row policies.  Tolerance: the 1e-12
relative-to-max of the apply tests.  (Every lane count, on synthetic matrices: test_conform_lanes_gpu.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import scipy.sparse as sp  # noqa: E402

from palace_amd import linalg  # noqa: E402
from palace_amd.fem import nchex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from tests import nc_util as nu  # noqa: E402

TOL = 1e-12
CASES = [(m, "nd", p) for m in "AC" for p in (1, 2, 3, 4, 5)] + [(m, "h1", p) for m in "AC" for p in (1, 2, 3)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _relmax(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


def _setup(ctx, name, kind, p):
    s = nu.nc_space(name, kind, p)
    rng = np.random.default_rng(100 * p + len(kind) + ord(name))
    ess = s.ess_dofs()
    mask = np.zeros(s.n_true, dtype=np.uint8)
    mask[ess] = 1
    return s, linalg.Conforming(ctx, s), rng, mask


@pytest.mark.parametrize("name,kind,p", CASES)
def test_prolongate(ctx, name, kind, p):
    s, c, rng, mask = _setup(ctx, name, kind, p)
    assert c.n_true == s.n_true and c.n_local == s.n_local
    longest = int(np.diff(s.C.indptr).max())
    assert c.lanes() == min(32, 1 << max(0, longest - 1).bit_length())   # one power-of-two lane group per row
    P = s.prolongation()
    x = rng.uniform(-1, 1, s.n_true)
    for m in (None, mask):
        lx = torch.full((s.n_local,), np.nan, dtype=torch.float64, device="cuda")
        c.prolongate(_dev(x), lx, None if m is None else _dev(m))
        tx = x.copy()
        if m is not None:
            tx[m != 0] = 0.0
        ref = P @ tx
        got = lx.cpu().numpy()
        print(f"{name} {kind} p={p} masked={m is not None}: {_relmax(got, ref):.2e}")
        assert _relmax(got, ref) < TOL
        assert np.array_equal(got[:s.n_true], tx)   # the head is a copy


@pytest.mark.parametrize("name,kind,p", CASES)
def test_restrict(ctx, name, kind, p):
    s, c, rng, mask = _setup(ctx, name, kind, p)
    P = s.prolongation()
    ly = rng.uniform(-1, 1, s.n_local)
    y0 = rng.uniform(-1, 1, s.n_true)
    xe = rng.uniform(-1, 1, s.n_true)
    d_ly, d_mask, d_xe = _dev(ly), _dev(mask), _dev(xe)
    on = mask != 0
    for absolute in (False, True):
        base = (abs(P) if absolute else P).T @ ly
        fl_abs = c.ABS if absolute else 0
        for fix in (0, c.FIX_ONE, c.FIX_ZERO):
            v = base.copy()
            if fix:
                v[on] = xe[on] if fix == c.FIX_ONE else 0.0
            for add, a in ((False, 1.0), (True, -0.75)):
                y = _dev(y0.copy())
                c.restrict(d_ly, y, fl_abs | fix | (c.ADD if add else 0), a, d_mask if fix else None, d_xe if fix == c.FIX_ONE else None)
                ref = y0 + a * v if add else v
                got = y.cpu().numpy()
                err = _relmax(got, ref)
                assert err < TOL, (absolute, fix, add, err)
                if fix == c.FIX_ONE and not add:
                    assert np.array_equal(got[on], xe[on])   # DIAG_ONE rows: a bit-exact copy
    # the gather runs in a fixed order: two calls give the same bits
    ya, yb = torch.zeros(s.n_true, dtype=torch.float64, device="cuda"), torch.ones(s.n_true, dtype=torch.float64, device="cuda")
    c.restrict(d_ly, ya)
    c.restrict(d_ly, yb)
    assert torch.equal(ya, yb)
    assert c.lanes(True) == min(32, 1 << max(0, int(np.diff(s.C.tocsc().indptr).max()) - 1).bit_length())


def test_restrict_in_place_on_x(ctx):
    """ParOperator::Mult may be called with y = x: the essential rows read x[i] where they write y[i]."""
    s, c, rng, mask = _setup(ctx, "A", "nd", 2)
    ly, x = rng.uniform(-1, 1, s.n_local), rng.uniform(-1, 1, s.n_true)
    xy = _dev(x.copy())
    c.restrict(_dev(ly), xy, c.FIX_ONE, 1.0, _dev(mask), xy)
    ref = s.prolongation().T @ ly
    ref[mask != 0] = x[mask != 0]
    assert _relmax(xy.cpu().numpy(), ref) < TOL


def test_unaligned_views(ctx):
    """Vectors that do not start on a 16-byte boundary take the scalar head copy."""
    s, c, rng, mask = _setup(ctx, "A", "h1", 2)
    P = s.prolongation()
    x, ly = rng.uniform(-1, 1, s.n_true), rng.uniform(-1, 1, s.n_local)
    bx, blx = torch.zeros(s.n_true + 1, dtype=torch.float64, device="cuda"), torch.zeros(s.n_local + 1, dtype=torch.float64, device="cuda")
    bx[1:] = _dev(x)
    c.prolongate(bx[1:], blx[1:])
    assert _relmax(blx[1:].cpu().numpy(), P @ x) < TOL and blx[0].item() == 0.0
    by = torch.zeros(s.n_true + 1, dtype=torch.float64, device="cuda")
    blx[1:] = _dev(ly)
    c.restrict(blx[1:], by[1:])
    assert _relmax(by[1:].cpu().numpy(), P.T @ ly) < TOL and by[0].item() == 0.0


def test_no_constraints_is_the_identity(ctx):
    """A conforming mesh: zero rows, both products copy."""
    s = nchex.NCSpace(NDHexSpace(nchex.refine_local(nu.start_mesh("A"), []), 2))
    assert s.C.shape == (0, s.n_true)
    c = linalg.Conforming(ctx, s)
    x = np.random.default_rng(0).uniform(-1, 1, s.n_true)
    lx = torch.zeros(s.n_true, dtype=torch.float64, device="cuda")
    c.prolongate(_dev(x), lx)
    assert np.array_equal(lx.cpu().numpy(), x)
    y = torch.zeros(s.n_true, dtype=torch.float64, device="cuda")
    c.restrict(lx, y)
    assert np.array_equal(y.cpu().numpy(), x)


def test_bad_input_is_refused(ctx):
    """A column that is not a true dof (a chain of constraints) is an error, not an out-of-range read."""
    bad = sp.csr_matrix((np.ones(2), (np.array([0, 0]), np.array([1, 5]))), shape=(1, 6))
    with pytest.raises(Exception, match="true dof"):
        linalg.Conforming(ctx, bad, n_true=4, n_local=5)
