"""The two-vector form of the conforming prolongation (pa_conform.hip: Prolongate2 / Restrict2, both parts of a complex field in
one launch: the kernels' TWO = true instantiations) against the one-vector form of the same kernels, part by part and bit for
bit: same lane assignment, same summation order.  Every flag combination of test_conform_gpu.py, aligned and misaligned
pointers, the identity object and repeats."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from palace_amd import linalg  # noqa: E402
from palace_amd.fem import nchex, rthex  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import rt_nc_util as rn  # noqa: E402
from tests.nc_util import shifted as _shifted  # noqa: E402

CASES = [("A", "nd", 2), ("A", "rt", 1), ("A", "rt", 3), ("C", "rt", 2)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


def _setup(ctx, name, kind, p):
    s = rn.rt_space(name, p) if kind == "rt" else nu.nc_space(name, kind, p)
    rng = np.random.default_rng(100 * p + len(kind) + ord(name))
    mask = np.zeros(s.n_true, dtype=np.uint8)
    ess = s.ess_dofs()
    if ess.size == 0:  # an RT space has no essential dofs: a seeded tenth, so that the masked paths run
        ess = np.nonzero(rng.uniform(0, 1, s.n_true) < 0.1)[0]
    mask[ess] = 1
    return s, linalg.Conforming(ctx, s), rng, mask


@pytest.mark.parametrize("name,kind,p", CASES)
@pytest.mark.parametrize("off", [(0, 0), (1, 1), (0, 1)])
def test_prolongate2(ctx, name, kind, p, off):
    s, c, rng, mask = _setup(ctx, name, kind, p)
    x = [rng.uniform(-1, 1, s.n_true) for _ in range(2)]
    for m in (None, _dev(mask)):
        one = []
        for k in range(2):
            lx = torch.full((s.n_local + off[k],), np.nan, dtype=torch.float64, device="cuda")[off[k]:]
            one.append(c.prolongate(_shifted(x[k], off[k]), lx, m).cpu().numpy())
        for rep in range(2):
            lx = [torch.full((s.n_local + off[k],), np.nan, dtype=torch.float64, device="cuda")[off[k]:] for k in range(2)]
            c.prolongate2(_shifted(x[0], off[0]), _shifted(x[1], off[1]), lx[0], lx[1], m)
            for k in range(2):
                assert np.array_equal(lx[k].cpu().numpy(), one[k]), (m is not None, rep, k)
    assert np.all(np.isfinite(one[0])) and np.any(one[0][s.n_true:] != 0.0)


@pytest.mark.parametrize("name,kind,p", CASES)
@pytest.mark.parametrize("off", [(0, 0), (1, 1), (1, 0)])
def test_restrict2(ctx, name, kind, p, off):
    s, c, rng, mask = _setup(ctx, name, kind, p)
    ly = [rng.uniform(-1, 1, s.n_local) for _ in range(2)]
    y0 = [rng.uniform(-1, 1, s.n_true) for _ in range(2)]
    xe = [rng.uniform(-1, 1, s.n_true) for _ in range(2)]
    d_ly = [_shifted(ly[k], off[k]) for k in range(2)]
    d_xe = [_dev(xe[k]) for k in range(2)]
    d_mask = _dev(mask)
    for absolute in (False, True):
        for fix in (0, c.FIX_ONE, c.FIX_ZERO):
            for add, a in ((False, 1.0), (True, -0.75)):
                flags = (c.ABS if absolute else 0) | fix | (c.ADD if add else 0)
                m = d_mask if fix else None
                e = d_xe if fix == c.FIX_ONE else [None, None]
                one = [c.restrict(d_ly[k], _shifted(y0[k], off[k]), flags, a, m, e[k]).cpu().numpy() for k in range(2)]
                for rep in range(2):
                    y = [_shifted(y0[k], off[k]) for k in range(2)]
                    c.restrict2(d_ly[0], d_ly[1], y[0], y[1], flags, a, m, e[0], e[1])
                    for k in range(2):
                        assert np.array_equal(y[k].cpu().numpy(), one[k]), (absolute, fix, add, rep, k)
    assert np.all(np.isfinite(one[0]))


def test_restrict2_in_place_on_x(ctx):
    """As ParOperator::Mult may call it with y = x: the essential rows read x[i] where they write y[i]."""
    s, c, rng, mask = _setup(ctx, "A", "nd", 2)
    ly = [_dev(rng.uniform(-1, 1, s.n_local)) for _ in range(2)]
    x = [rng.uniform(-1, 1, s.n_true) for _ in range(2)]
    m = _dev(mask)
    one = []
    for k in range(2):
        xy = _dev(x[k].copy())
        one.append(c.restrict(ly[k], xy, c.FIX_ONE, 1.0, m, xy).cpu().numpy())
    xy = [_dev(x[k].copy()) for k in range(2)]
    c.restrict2(ly[0], ly[1], xy[0], xy[1], c.FIX_ONE, 1.0, m, xy[0], xy[1])
    for k in range(2):
        assert np.array_equal(xy[k].cpu().numpy(), one[k])
        assert np.array_equal(one[k][mask != 0], x[k][mask != 0])


def test_no_constraints_is_the_identity(ctx):
    """A conforming mesh: zero rows, both products copy both parts."""
    s = nchex.NCSpace(rthex.RTHexSpace(nchex.refine_local(nu.start_mesh("A"), []), 2))
    assert s.C.shape == (0, s.n_true)
    c = linalg.Conforming(ctx, s)
    x = [np.random.default_rng(k).uniform(-1, 1, s.n_true) for k in range(2)]
    lx = [torch.zeros(s.n_true, dtype=torch.float64, device="cuda") for _ in range(2)]
    c.prolongate2(_dev(x[0]), _dev(x[1]), lx[0], lx[1])
    y = [torch.zeros(s.n_true, dtype=torch.float64, device="cuda") for _ in range(2)]
    c.restrict2(lx[0], lx[1], y[0], y[1])
    for k in range(2):
        assert np.array_equal(lx[k].cpu().numpy(), x[k]) and np.array_equal(y[k].cpu().numpy(), x[k])


def test_overlapping_outputs_are_refused(ctx):
    """Two parts written to one buffer would race: an error, not a wrong answer."""
    s, c, rng, _ = _setup(ctx, "A", "rt", 1)
    x = _dev(rng.uniform(-1, 1, s.n_true))
    lx = torch.zeros(s.n_local, dtype=torch.float64, device="cuda")
    with pytest.raises(Exception, match="overlap"):
        c.prolongate2(x, x, lx, lx)
    y = torch.zeros(s.n_true, dtype=torch.float64, device="cuda")
    with pytest.raises(Exception, match="overlap"):
        c.restrict2(lx, lx, y, y)
