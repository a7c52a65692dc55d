"""Ready-made index words of the compact-only streaming H(curl) hex kernels (pa_nd_hex_stream.hip, COMPACT): the kernel reads
the signed sorted index of every entry from a plain table (pack_index_plain) and keeps the batch's index, slot and flag words in
registers up to the E^T stores.  PALACE_AMD_STREAM_COMPACT=0 (read at every launch) runs the general form, which decodes the
run-compressed index of the same operator and parks the words in LDS: an independent decode of the same tables, so the two must
agree bit for bit (torch.equal).  The mesh is the smallest extruded O-grid -- 15 elements, so the last batch holds three elements
and a pad element, and four batches, far fewer than waves: every wave's first batch is its last -- with every element handed over
in one of the eight rotations that keep its local zeta along the extrusion (negative index words, many orientations of the shared
faces and edges); a second numbering exchanges single interior dofs between far blocks until an element's run count reaches the
capacity of the compressed block."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import HexMesh, ogrid_cylinder  # noqa: E402
from tests import util  # noqa: E402

RTOL = 1e-12  # against the C oracle: the suite's bound (tests/test_apply_gpu.py)
Q1D = 4
FORMS = ["curl_packed", "mass_packed", "km_packed12", "km_metric"]
SWITCH = "PALACE_AMD_STREAM_COMPACT"
CAP = 20  # kIdxMaxRuns of pa_stream_host.hpp


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


class _Mesh:
    def __init__(self):
        base = ogrid_cylinder(1, 3)
        base = HexMesh(x=base.x.copy(), elem_nodes=base.elem_nodes, attr=(np.arange(base.ne) % 3 + 1).astype(np.int32))
        base.check()
        assert base.ne == 15
        # the rotations that map local zeta to +-zeta: the element stays separable along its zeta (the rule is symmetric)
        mats, _ = util.hex_rotations()
        keep = np.array([i for i in range(24) if abs(mats[i][2, 2]) == 1])
        assert keep.size == 8
        self.mesh = util.rotate_elements(base, keep[np.random.default_rng(3).permutation(np.arange(base.ne) % 8)])
        self.ogeom = util.oracle_geom(self.mesh, Q1D)
        self.spaces = {p: NDHexSpace(self.mesh, p) for p in (1, 2, 3)}
        self._ref = {}

    def oracle(self, p, qf, blob, x):
        key = (p, qf, blob.tobytes(), x.tobytes())
        if key not in self._ref:
            self._ref[key] = util.oracle_apply_c(self.spaces[p], self.ogeom, qf, blob, x, Q1D)
        return self._ref[key]


@pytest.fixture(scope="module")
def M():
    return _Mesh()


def _build(geom, nd, form):
    _, b_a = util.make_ctx("aniso", nattr=3)
    _, b_s = util.make_ctx("scalar", nattr=3)
    if form == "curl_packed":
        return ceed.curlcurl_operator(geom, nd, b_a), "hdiv", b_a
    if form == "mass_packed":
        return ceed.ndmass_operator(geom, nd, b_a), "hcurl", b_a
    if form == "km_metric":
        return ceed.curlcurlmass_operator(geom, nd, b_s, b_s), "hdivmass", np.concatenate([b_s, b_s])
    return ceed.curlcurlmass_operator(geom, nd, b_a, b_a), "hdivmass", np.concatenate([b_a, b_a])


def _operator(M, nd, form):
    geom = ceed.GeomFactorData(M.mesh, Q1D)
    op, qf, blob = _build(geom, nd, form)
    return geom, op, qf, blob


def _on_off(monkeypatch, fn):
    """fn() on the plain index (the default) and on the general form's compressed decode, same objects, same process"""
    monkeypatch.delenv(SWITCH, raising=False)
    on = fn()
    monkeypatch.setenv(SWITCH, "0")
    off = fn()
    monkeypatch.delenv(SWITCH)
    return on, off


def _flipped_essential(nd):
    """essential dofs, with the check that some element holds one of them flipped (a negative index word under the mask)"""
    ess = nd.ess_dofs()
    mask = np.zeros(nd.ndofs, dtype=bool)
    mask[ess] = True
    assert (mask[nd.elem_dof_lex] & (nd.elem_sign_lex < 0)).any()
    return ess


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_plain_index_equals_compressed_decode(M, monkeypatch, p, form):
    """y = A x and the masked apply with the fix-up fused (an essential list that holds a flipped entry)."""
    nd = M.spaces[p]
    n = nd.ndofs
    assert (nd.elem_sign_lex < 0).any()
    geom, op, qf, blob = _operator(M, nd, form)
    assert op.streams() and op.stream_compact()
    x = np.random.default_rng(20 + p).uniform(-1, 1, n)
    xd = _dev(x)
    y, y0 = _on_off(monkeypatch, lambda: op.mult(xd, _nan(n)).clone())
    print(f"{form} p={p}: plain against compressed index, largest difference {float((y - y0).abs().max()):.2e}")
    assert torch.equal(y, y0)
    err = _rel(y.cpu().numpy(), M.oracle(p, qf, blob, x))
    print(f"{form} p={p}: against the oracle {err:.2e}")
    assert err < RTOL
    ess = _flipped_essential(nd)
    K = linalg.ParOperator(linalg.Context(), op, ess, linalg.DIAG_ONE)
    yk, yk0 = _on_off(monkeypatch, lambda: K.mult(xd, _nan(n)).clone())
    assert torch.equal(yk, yk0)
    xm = x.copy()
    xm[ess] = 0.0
    refk = M.oracle(p, qf, blob, xm).copy()
    refk[ess] = x[ess]
    assert _rel(yk.cpu().numpy(), refk) < RTOL


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", ["curl_packed", "km_metric"])
def test_split_vectors(M, monkeypatch, p, form):
    """The split-vector instantiations (true dofs and ghosts through two base pointers) against the plain apply, both indices."""
    nd = M.spaces[p]
    n, n_true = nd.ndofs, int(0.7 * nd.ndofs)
    geom, op, qf, blob = _operator(M, nd, form)
    assert op.stream_compact() and op.supports_split()
    x = _dev(np.random.default_rng(30 + p).uniform(-1, 1, n))
    ref = op.mult(x, torch.empty_like(x))

    def split():
        y = _nan(n_true)
        yg = torch.zeros(n - n_true, dtype=torch.float64, device="cuda")
        op.mult_split(x[:n_true].clone(), x[n_true:].clone(), y, yg)
        return torch.cat([y, yg])

    s, s0 = _on_off(monkeypatch, split)
    assert torch.equal(s, ref) and torch.equal(s0, ref)


@pytest.mark.parametrize("first_kind", [False, True])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", ["km_packed12", "km_metric"])
def test_fused_chebyshev_step_and_residual(M, monkeypatch, p, form, first_kind):
    """The `all` copy of the flag words (no entry goes straight to y): the smoother step and the residual in the epilogue of the
    E^T gather, zero and non-zero initial guess."""
    nd = M.spaces[p]
    n = nd.ndofs
    geom, op, qf, blob = _operator(M, nd, form)
    assert op.stream_compact()
    ctx = linalg.Context()
    ess = _flipped_essential(nd)
    A = linalg.ParOperator(ctx, op, ess, linalg.DIAG_ONE)
    S = linalg.chebyshev(ctx, A, order=4, fourth_kind=not first_kind)
    assert S.fused_step()
    rng = np.random.default_rng(40)
    b, g = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b[ess] = 0.0
    g[ess] = 0.0
    y, y0 = _on_off(monkeypatch, lambda: S.mult(_dev(b), torch.zeros(n, dtype=torch.float64, device="cuda")).clone())
    z, z0 = _on_off(monkeypatch, lambda: S.mult(_dev(b), _dev(g.copy()), initial_guess=True).clone())
    assert torch.equal(y, y0) and torch.equal(z, z0)
    assert torch.isfinite(y).all() and torch.isfinite(z).all() and float(y.abs().max()) > 0.0


@pytest.mark.parametrize("form", ["curl_packed", "km_metric"])
@pytest.mark.parametrize("over", [0, 2])
def test_fragmented_numbering(M, monkeypatch, form, over):
    """Order 3 with single interior dofs exchanged between far blocks of the numbering until an element has 19 or 20 runs (a
    compressed block at its capacity, many runs of one entry: the plain table names the same dofs) or 21 or 22 (more than the
    block holds: the operator keeps the one-shot kernel, with or without the plain table)."""
    nd = M.spaces[3]
    n = nd.ndofs
    geom, op, qf, blob = _operator(M, nd, form)
    x = np.random.default_rng(50).uniform(-1, 1, n)
    y_nat = op.mult(_dev(x), _nan(n)).cpu().numpy()
    perm, runs = util.fragmenting_permutation(nd, "interior", CAP + over)
    # (every exchange adds two runs to an element: the count lands on the target or one below it)
    assert CAP + over - 1 <= runs.max() <= CAP + over and util.element_runs(nd.elem_dof_lex).max() < CAP - 1
    space = util.renumbered(nd, perm)
    opf = _build(geom, space, form)[0]
    assert opf.streams() == (over == 0)
    xp = np.empty(n)
    xp[perm] = x
    if over:
        assert not opf.stream_compact()
        yp = opf.mult(_dev(xp), _nan(n)).cpu().numpy()
        assert np.abs(yp[perm] - y_nat).max() <= 1e-13 * np.abs(y_nat).max()  # (another schedule: tests/test_orient_gpu.py)
        return
    assert opf.stream_compact()
    yp, yp0 = _on_off(monkeypatch, lambda: opf.mult(_dev(xp), _nan(n)).clone())
    assert torch.equal(yp, yp0)
    assert np.array_equal(yp.cpu().numpy()[perm], y_nat)  # the same kernel, the same sums under another naming of the dofs
