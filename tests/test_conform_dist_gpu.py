"""The conforming prolongation that carries its halo (pa_conform_create_dist, palace_amd/csrc/pa_conform.hip): P = [I; C] P_halo
and its transpose in pieces around the exchange.  With one rank and an empty halo the pieces reproduce the one-launch kernels
bit for bit; across ranks (threads over linalg.LocalGroup) every product equals the global scipy P restricted to the rank's
dofs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from palace_amd import linalg  # noqa: E402
from tests import nc_ranks_util as ru  # noqa: E402
from tests import nc_util as nu  # noqa: E402

ADD, ABS, ONE, ZERO = (linalg.Conforming.ADD, linalg.Conforming.ABS, linalg.Conforming.FIX_ONE, linalg.Conforming.FIX_ZERO)
# (flags, with the essential mask)
FLAGS = [(0, False), (ADD, False), (ABS, False), (ABS | ADD, False), (ONE, True), (ZERO, True), (ADD | ONE, True),
         (ADD | ZERO, True), (0, True)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _mask(n, ess):
    m = np.zeros(n, dtype=np.uint8)
    m[np.asarray(ess, dtype=np.int64)] = 1
    return m


@pytest.mark.parametrize("name,kind,p", [("A", "nd", 1), ("A", "nd", 2), ("A", "h1", 2), ("B", "nd", 2), ("B", "nd", 3), ("B", "h1", 2)])
def test_one_rank_empty_halo_is_the_plain_object(name, kind, p):
    """world = 1: array_equal with pa_conform_create's kernels, every flag combination and the two-vector forms."""
    s = nu.nc_space(name, kind, p)
    ctx = linalg.Context()
    plain = linalg.Conforming(ctx, s)
    dist = linalg.Conforming(ctx, s, n_shared=s.n_true)
    assert (dist.n_true, dist.n_shared, dist.n_local) == (s.n_true, s.n_true, s.n_local)
    assert dist.lanes() == plain.lanes() and dist.lanes(True) == plain.lanes(True)
    n, nl = s.n_true, s.n_local
    rng = np.random.default_rng(p)
    x0, x1, ly0, ly1 = (_dev(rng.uniform(-1, 1, m)) for m in (n, n, nl, nl))
    yi0, yi1, xe0, xe1 = (rng.uniform(-1, 1, n) for _ in range(4))
    mask = _dev(_mask(n, s.ess_dofs()))
    for m in (None, mask):
        a = plain.prolongate(x0, _new(nl), m)
        b = dist.prolongate(x0, _new(nl), m)
        assert torch.equal(a, b)
        b0, b1 = dist.prolongate2(x0, x1, _new(nl), _new(nl), m)
        assert torch.equal(b0, a) and torch.equal(b1, plain.prolongate(x1, _new(nl), m))
    for flags, masked in FLAGS:
        m = mask if masked else None
        a0 = plain.restrict(ly0, _dev(yi0), flags, -0.75, m, _dev(xe0))
        a1 = plain.restrict(ly1, _dev(yi1), flags, -0.75, m, _dev(xe1))
        b0 = dist.restrict(ly0, _dev(yi0), flags, -0.75, m, _dev(xe0))
        assert torch.equal(a0, b0), flags
        c0, c1 = dist.restrict2(ly0, ly1, _dev(yi0), _dev(yi1), flags, -0.75, m, _dev(xe0), _dev(xe1))
        assert torch.equal(c0, a0) and torch.equal(c1, a1), flags
    # y may be x_ess (ParOperator::Mult in place)
    y = _dev(xe0)
    assert torch.equal(dist.restrict(ly0, y, ONE, 1.0, mask, y), plain.restrict(ly0, _dev(yi0), ONE, 1.0, mask, _dev(xe0)))


def _close(got, want, scale):
    return np.max(np.abs(got - want)) <= 1e-13 * scale


def _rank_products(name, kind, p, how):
    s, vs = ru.views(name, kind, p, how)
    world = len(vs)
    Pg = s.prolongation()
    rng = np.random.default_rng(7 * p + world)
    x, x1 = rng.uniform(-1, 1, s.n_true), rng.uniform(-1, 1, s.n_true)
    ess_g = np.asarray(s.ess_dofs(), dtype=np.int64)
    xm = x.copy()
    xm[ess_g] = 0.0
    lys = [(rng.uniform(-1, 1, v.n_local), rng.uniform(-1, 1, v.n_local)) for v in vs]
    lg = [np.zeros(s.ndofs), np.zeros(s.ndofs)]
    for v, l in zip(vs, lys):
        for k in (0, 1):
            np.add.at(lg[k], v.l2g, l[k])
    yin, xe = rng.uniform(-1, 1, s.n_true), rng.uniform(-1, 1, s.n_true)
    is_ess = np.zeros(s.n_true, dtype=bool)
    is_ess[ess_g] = True

    def want(flags, masked, k):
        t = (abs(Pg) if flags & ABS else Pg).T @ lg[k]
        if masked and flags & (ONE | ZERO):
            t = np.where(is_ess, xe if flags & ONE else 0.0, t)
        return yin - 0.75 * t if flags & ADD else t

    def rank_main(ctx, rank):
        v = vs[rank]
        conf, halo = ru.rank_conforming(ctx, v, world)
        assert (conf.n_true, conf.n_shared, conf.n_local) == (v.n_true, v.n_shared, v.n_local)
        own = v.l2g[:v.n_true]
        mask = _dev(_mask(v.n_true, v.ess_dofs()))
        res = {}
        # P x, with and without the essential mask (the ghost copies of essential dofs are zero too)
        for m, xx in ((None, x), (mask, xm)):
            lx = conf.prolongate(_dev(x[own]), _new(v.n_local), m)
            assert _close(lx.cpu().numpy(), (Pg @ xx)[v.l2g], 1.0), ("prolongate", m is not None)
            again = conf.prolongate(_dev(x[own]), _new(v.n_local), m)
            assert torch.equal(lx, again)
            l0, l1 = conf.prolongate2(_dev(x[own]), _dev(x1[own]), _new(v.n_local), _new(v.n_local), m)
            assert torch.equal(l0, lx) and torch.equal(l1, conf.prolongate(_dev(x1[own]), _new(v.n_local), m))
        ly0, ly1 = _dev(lys[rank][0]), _dev(lys[rank][1])
        for flags, masked in FLAGS:
            m = mask if masked else None
            y0 = conf.restrict(ly0, _dev(yin[own]), flags, -0.75, m, _dev(xe[own]))
            y1 = conf.restrict(ly1, _dev(yin[own]), flags, -0.75, m, _dev(xe[own]))
            for k, y in ((0, y0), (1, y1)):
                w = want(flags, masked, k)
                assert _close(y.cpu().numpy(), w[own], max(1.0, np.max(np.abs(w)))), ("restrict", flags, k)
            assert torch.equal(y0, conf.restrict(ly0, _dev(yin[own]), flags, -0.75, m, _dev(xe[own]))), flags
            c0, c1 = conf.restrict2(ly0, ly1, _dev(yin[own]), _dev(yin[own]), flags, -0.75, m, _dev(xe[own]), _dev(xe[own]))
            assert torch.equal(c0, y0) and torch.equal(c1, y1), flags
        assert torch.equal(ly0, _dev(lys[rank][0]))  # the caller's local vector stays as it was
        res["n_true"] = v.n_true
        return res

    out = ru.run_ranks(world, rank_main)
    assert sum(o["n_true"] for o in out) == s.n_true


@pytest.mark.parametrize("how", ["rcb2", "rcb3", "hand"])
@pytest.mark.parametrize("kind,p", [("nd", 2), ("h1", 2), ("nd", 3)])
def test_ranks_against_the_global_prolongation(kind, p, how):
    """Mesh A on 2 and 3 ranks (the hand partition has dependency-only ghosts on rank 0 and no constrained dof on rank 1)."""
    _rank_products("A", kind, p, how)


def test_bad_arguments_are_refused():
    s = nu.nc_space("A", "nd", 2)
    ctx = linalg.Context()
    with pytest.raises(Exception, match="halo"):
        linalg.Conforming(ctx, s.C, n_true=s.n_true - 1, n_shared=s.n_true)     # ghosts without a plan
    with pytest.raises(Exception, match="bad sizes"):
        linalg.Conforming(ctx, s.C, n_true=s.n_true + 1, n_shared=s.n_true)
