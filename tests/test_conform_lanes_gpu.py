"""Every lane count of the conforming prolongation kernels (palace_amd/csrc/pa_conform.hip) on synthetic constraint matrices:
the meshes of the other conforming tests never give a transposed lane group of 1 or 2, and reach the kernels of the halo-carrying
object with few lane counts and aligned vectors only.  linalg.Conforming takes a raw scipy CSR, so each case builds a seeded C
with a chosen longest row and fullest column and first asserts the lane counts it was built for.

n_true = 1031 (odd: the scalar tail of the pair copy runs; above 512: several head blocks), 300 constrained rows (with one lane
per row the row part spans two blocks).  Per case, once with aligned vectors and once with every vector one double past a
16-byte boundary:
  * prolongate (masked and not) and restrict (every flag combination of test_conform_dist_gpu.py) against scipy, the
    relative-to-max 1e-12 of test_conform_gpu.py;
  * the two-vector calls against the one-vector calls, array_equal;
  * the halo-less distributed object (n_shared = n_true) against the plain object, array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import scipy.sparse as sp  # noqa: E402

from palace_amd import linalg  # noqa: E402
from tests.nc_util import shifted  # noqa: E402
from tests.test_conform_dist_gpu import ABS, ADD, FLAGS, ONE, ZERO  # noqa: E402

TOL = 1e-12
N_TRUE, N_CON = 1031, 300
PAIRS = [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (32, 32), (32, 1), (1, 32)]   # (forward lanes, transposed lanes)
_cache = {}


def constraint_matrix(l_fwd, l_tr):
    """Seeded C [N_CON, N_TRUE] whose longest row takes l_fwd lanes and whose fullest column takes l_tr lanes."""
    key = (l_fwd, l_tr)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * l_fwd + l_tr)
    if l_fwd == l_tr:
        # row lengths in [1, L], one row full; the fullest column (`hot`) holds L/2 + 1 .. L entries, no column more than L
        L = l_fwd
        lens = rng.integers(1, L + 1, N_CON)
        lens[rng.integers(N_CON)] = L
        hot = int(rng.integers(N_TRUE))
        hot_rows = set(rng.choice(N_CON, size=int(rng.integers(L // 2 + 1, L + 1)), replace=False).tolist())
        count = np.zeros(N_TRUE, dtype=np.int64)
        count[hot] = L   # placed by hand below
        rows = []
        for r in range(N_CON):
            own = [hot] if r in hot_rows else []
            cols = np.concatenate([own, rng.choice(np.nonzero(count < L)[0], size=lens[r] - len(own), replace=False)]).astype(np.int64)
            count[cols[len(own):]] += 1
            rows.append(np.sort(cols))
    elif l_tr == 1:
        # one long row, every other row one column, all columns distinct
        k = int(rng.integers(l_fwd // 2 + 1, l_fwd + 1))
        cols = rng.permutation(N_TRUE)[:k + N_CON - 1]
        rows = [cols[k + r:k + r + 1] for r in range(N_CON - 1)]
        rows.insert(int(rng.integers(N_CON)), np.sort(cols[:k]))
    else:
        # one entry per row, one column shared by l_tr / 2 + 1 .. l_tr rows
        assert l_fwd == 1
        k = int(rng.integers(l_tr // 2 + 1, l_tr + 1))
        cols = rng.permutation(N_TRUE)[:N_CON - k + 1]
        col_of_row = np.concatenate([np.full(k, cols[0]), cols[1:]])[rng.permutation(N_CON)]
        rows = [col_of_row[r:r + 1] for r in range(N_CON)]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])])
    indices = np.concatenate(rows)
    sign = np.where(rng.uniform(0, 1, indices.size) < 0.5, -1.0, 1.0)   # both signs, none near zero: ABS is seen
    Cm = sp.csr_matrix((sign * rng.uniform(0.25, 1.0, indices.size), indices, indptr), shape=(N_CON, N_TRUE))
    _cache[key] = Cm
    return Cm


def _relmax(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("l_fwd,l_tr", PAIRS)
def test_lane_pair(ctx, l_fwd, l_tr, off):
    Cm = constraint_matrix(l_fwd, l_tr)
    n, nl = N_TRUE, N_TRUE + N_CON
    plain = linalg.Conforming(ctx, Cm)
    dist = linalg.Conforming(ctx, Cm, n_shared=n)
    for c in (plain, dist):
        assert (c.n_true, c.n_shared, c.n_local) == (n, n, nl)
        assert c.lanes() == l_fwd and c.lanes(True) == l_tr   # the construction hit the kernels it is meant for
    P = sp.vstack([sp.identity(n, format="csr"), Cm]).tocsr()
    rng = np.random.default_rng(7 + 100 * l_fwd + l_tr)
    x, ly = rng.uniform(-1, 1, (2, n)), rng.uniform(-1, 1, (2, nl))
    yin, xe = rng.uniform(-1, 1, (2, n)), rng.uniform(-1, 1, (2, n))
    is_ess = rng.uniform(0, 1, n) < 0.15
    is_ess[Cm.indices[::7]] = True   # masters among the essential dofs: the masked reads of the row part
    mask = _dev(is_ess.astype(np.uint8))

    def dv(a):
        return shifted(a, off)

    def out(size):
        return torch.full((size + off,), np.nan, dtype=torch.float64, device="cuda")[off:]

    worst = 0.0
    for m in (None, mask):
        one = [plain.prolongate(dv(x[k]), out(nl), m).cpu().numpy() for k in (0, 1)]
        for k in (0, 1):
            ref = P @ (np.where(is_ess, 0.0, x[k]) if m is not None else x[k])
            worst = max(worst, _relmax(one[k], ref))
            assert _relmax(one[k], ref) < TOL, ("prolongate", m is not None, k)
            assert np.array_equal(one[k][:n], ref[:n])   # the head is a copy
            assert np.array_equal(dist.prolongate(dv(x[k]), out(nl), m).cpu().numpy(), one[k]), ("dist", m is not None, k)
        for c in (plain, dist):
            two = c.prolongate2(dv(x[0]), dv(x[1]), out(nl), out(nl), m)
            for k in (0, 1):
                assert np.array_equal(two[k].cpu().numpy(), one[k]), ("prolongate2", c is dist, m is not None, k)
    d_ly = [dv(ly[k]) for k in (0, 1)]
    for flags, masked in FLAGS:
        m = mask if masked else None
        one = [plain.restrict(d_ly[k], dv(yin[k]), flags, -0.75, m, dv(xe[k])).cpu().numpy() for k in (0, 1)]
        for k in (0, 1):
            t = (abs(P) if flags & ABS else P).T @ ly[k]
            if masked and flags & (ONE | ZERO):
                t = np.where(is_ess, xe[k] if flags & ONE else 0.0, t)
            ref = yin[k] - 0.75 * t if flags & ADD else t
            worst = max(worst, _relmax(one[k], ref))
            assert _relmax(one[k], ref) < TOL, ("restrict", flags, k)
            got = dist.restrict(d_ly[k], dv(yin[k]), flags, -0.75, m, dv(xe[k])).cpu().numpy()
            assert np.array_equal(got, one[k]), ("dist", flags, k)
        for c in (plain, dist):
            two = c.restrict2(d_ly[0], d_ly[1], dv(yin[0]), dv(yin[1]), flags, -0.75, m, dv(xe[0]), dv(xe[1]))
            for k in (0, 1):
                assert np.array_equal(two[k].cpu().numpy(), one[k]), ("restrict2", c is dist, flags, k)
    for k in (0, 1):
        assert np.array_equal(d_ly[k].cpu().numpy(), ly[k])   # the caller's local vector stays as it was
    print(f"lanes ({l_fwd}, {l_tr}) off={off}: nnz {Cm.nnz}, worst relative-to-max error {worst:.2e}")
