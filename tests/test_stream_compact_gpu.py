"""Compact-only form of the streaming H(curl) hex kernel (four points per direction): on a mesh whose batches of four elements are
all affine or column batches the kernel that runs never reads per-point D -- one 8-byte request per component and lane, the two
values the D stage needs formed right ahead of it (pa_nd_hex_stream.hip: COMPACT).  It computes the general form's products from
the general form's table entries, so the two must agree bit for bit: every case below compares the operator with itself under
PALACE_AMD_STREAM_COMPACT=0 (read at every apply) with torch.equal, and with the C oracle at the suite's 1e-12
(tests/test_apply_gpu.py).  Meshes on which one batch keeps per-point data must report the general form and stay correct."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import HexMesh, ogrid_cylinder  # noqa: E402
from tests import util  # noqa: E402

RTOL = 1e-12
Q1D = 4
FORMS = ["curl_packed", "curl_metric", "mass_packed", "mass_metric", "km_packed12", "km_metric"]
SWITCH = "PALACE_AMD_STREAM_COMPACT"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _with_attr(mesh, x=None):
    m = HexMesh(x=mesh.x.copy() if x is None else x, elem_nodes=mesh.elem_nodes, attr=(np.arange(mesh.ne) % 3 + 1).astype(np.int32))
    m.check()
    return m


class _Mesh:
    """a mesh with its spaces and the oracle's geometry factors, built once per module"""

    def __init__(self, mesh):
        self.mesh = mesh
        self.ogeom = util.oracle_geom(mesh, Q1D)
        self.spaces = {p: NDHexSpace(mesh, p) for p in (1, 2, 3)}
        self._ref = {}

    def oracle(self, p, qf, blob, x, tag):
        key = (p, qf, blob.tobytes(), tag)
        if key not in self._ref:
            self._ref[key] = util.oracle_apply_c(self.spaces[p], self.ogeom, qf, blob, x, Q1D)
        return self._ref[key]


@pytest.fixture(scope="module")
def extruded():
    # 60 elements, 15 batches: the central block affine, the outer blocks curved in the plane and extruded along local zeta
    return _Mesh(_with_attr(ogrid_cylinder(2, 3)))


@pytest.fixture(scope="module")
def extruded15():
    # 15 elements: the last batch holds three elements and one pad entry
    return _Mesh(_with_attr(ogrid_cylinder(1, 3)))


@pytest.fixture(scope="module")
def bent():
    # the mid node of one vertical edge of element 40 (an outer block) moved in x: the elements around that edge are not
    # separable along zeta any more, their batches keep the per-point data
    base = ogrid_cylinder(2, 3)
    x = base.x.copy()
    e = 40
    xe = base.x[base.elem_nodes[e]]
    node = base.elem_nodes[e, 9]  # lattice (0, 0, 1): between the two ends of the edge xi = eta = 0
    assert np.allclose(xe[9, :2], 0.5 * (xe[0, :2] + xe[18, :2]))
    x[node, 0] += 0.05 * (xe[:, 0].max() - xe[:, 0].min())
    return _Mesh(_with_attr(base, x=x))


@pytest.fixture(scope="module")
def rotated():
    # every element handed over in one of its 24 rotations: the extrusion runs along local xi or eta in most of them
    base = _with_attr(ogrid_cylinder(2, 3))
    return _Mesh(util.rotate_elements(base, util.seeded_rotations(base.ne, 24)))


def _build(geom, nd, form):
    _, b_a = util.make_ctx("aniso", nattr=3)
    _, b_s = util.make_ctx("scalar", nattr=3)
    if form == "curl_packed":
        return ceed.curlcurl_operator(geom, nd, b_a), "hdiv", b_a
    if form == "curl_metric":  # (the caller has set PALACE_AMD_DSTAGE=metric)
        return ceed.curlcurl_operator(geom, nd, b_s), "hdiv", b_s
    if form == "mass_packed":
        return ceed.ndmass_operator(geom, nd, b_a), "hcurl", b_a
    if form == "mass_metric":  # (PALACE_AMD_DSTAGE=metric)
        return ceed.ndmass_operator(geom, nd, b_s), "hcurl", b_s
    if form == "km_metric":
        return ceed.curlcurlmass_operator(geom, nd, b_s, b_s), "hdivmass", np.concatenate([b_s, b_s])
    return ceed.curlcurlmass_operator(geom, nd, b_a, b_a), "hdivmass", np.concatenate([b_a, b_a])


def _operator(M, p, form, monkeypatch):
    if form.endswith("_metric"):
        monkeypatch.setenv("PALACE_AMD_DSTAGE", "metric")
    geom = ceed.GeomFactorData(M.mesh, Q1D)
    op, qf, blob = _build(geom, M.spaces[p], form)
    assert op.streams()
    return geom, op, qf, blob


def _on_off(monkeypatch, fn):
    """fn() with the compact form allowed and with the general form forced, same objects, same process"""
    monkeypatch.delenv(SWITCH, raising=False)
    on = fn()
    monkeypatch.setenv(SWITCH, "0")
    off = fn()
    monkeypatch.delenv(SWITCH)
    return on, off


def _apply_checks(M, p, form, monkeypatch, expect_compact):
    """plain and masked apply: compact on against off (bit for bit) and against the oracle"""
    nd = M.spaces[p]
    n = nd.ndofs
    geom, op, qf, blob = _operator(M, p, form, monkeypatch)
    assert op.stream_compact() == expect_compact
    monkeypatch.setenv(SWITCH, "0")
    assert not op.stream_compact()
    monkeypatch.delenv(SWITCH)
    x = np.random.default_rng(7 + p).uniform(-1, 1, n)
    xd = _dev(x)
    nan = lambda: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")  # noqa: E731
    y, y0 = _on_off(monkeypatch, lambda: op.mult(xd, nan()).clone())
    print(f"{form} p={p}: compact on against off, largest difference {float((y - y0).abs().max()):.2e} of {float(y0.abs().max()):.2e}")
    assert torch.equal(y, y0)
    ref = M.oracle(p, qf, blob, x, "plain")
    err = _rel(y.cpu().numpy(), ref)
    print(f"{form} p={p}: compact {op.stream_compact()}, vs oracle {err:.2e}")
    assert err < RTOL
    # masked apply with the fix-up fused (the masked copy of the flag words)
    ess = nd.ess_dofs()
    K = linalg.ParOperator(linalg.Context(), op, ess, linalg.DIAG_ONE)
    yk, yk0 = _on_off(monkeypatch, lambda: K.mult(xd, nan()).clone())
    assert torch.equal(yk, yk0)
    xm = x.copy()
    xm[ess] = 0.0
    refk = M.oracle(p, qf, blob, xm, "masked").copy()
    refk[ess] = x[ess]
    assert _rel(yk.cpu().numpy(), refk) < RTOL
    return op


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", FORMS)
def test_compact_form_equals_general_form(extruded, monkeypatch, p, form):
    """Every batch of the extruded O-grid is an affine or a column batch: the compact form runs, and gives the general form's bits
    (both kinds of batch occur: the central block's batches are affine) and the oracle's result."""
    op = _apply_checks(extruded, p, form, monkeypatch, True)
    col, aff = op.stream_column(), op.stream_affine()
    assert col[2] + aff[2] == 60 and col[2] > 0 and aff[2] > 0


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", ["curl_packed", "mass_packed", "km_packed12", "km_metric"])
def test_split_vectors(extruded, monkeypatch, p, form):
    """The split-vector instantiations (true dofs and ghosts through two base pointers) of the compact form against the plain
    apply, bit for bit, compact on and off."""
    nd = extruded.spaces[p]
    n, n_true = nd.ndofs, int(0.7 * nd.ndofs)
    geom, op, qf, blob = _operator(extruded, p, form, monkeypatch)
    assert op.stream_compact() and op.supports_split()
    x = _dev(np.random.default_rng(11 + p).uniform(-1, 1, n))
    ref = op.mult(x, torch.empty_like(x))

    def split():
        y = torch.full((n_true,), float("nan"), dtype=torch.float64, device="cuda")
        yg = torch.zeros(n - n_true, dtype=torch.float64, device="cuda")
        op.mult_split(x[:n_true].clone(), x[n_true:].clone(), y, yg)
        return torch.cat([y, yg])

    s, s0 = _on_off(monkeypatch, split)
    assert torch.equal(s, ref) and torch.equal(s0, ref)


@pytest.mark.parametrize("first_kind", [False, True])
@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("form", ["km_packed12", "km_metric"])
def test_fused_chebyshev_step_and_residual(extruded, monkeypatch, p, form, first_kind):
    """The `all` copy of the flag words: the smoother step and the residual evaluated in the epilogue of the E^T gather (zero and
    non-zero initial guess), the same smoother applied with the compact form on and off."""
    nd = extruded.spaces[p]
    n = nd.ndofs
    geom, op, qf, blob = _operator(extruded, p, form, monkeypatch)
    assert op.stream_compact()
    ctx = linalg.Context()
    A = linalg.ParOperator(ctx, op, nd.ess_dofs(), linalg.DIAG_ONE)
    S = linalg.chebyshev(ctx, A, order=4, fourth_kind=not first_kind)
    assert S.fused_step()
    rng = np.random.default_rng(16)
    b, g = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b[nd.ess_dofs()] = 0.0
    g[nd.ess_dofs()] = 0.0
    y, y0 = _on_off(monkeypatch, lambda: S.mult(_dev(b), torch.zeros(n, dtype=torch.float64, device="cuda")).clone())
    z, z0 = _on_off(monkeypatch, lambda: S.mult(_dev(b), _dev(g.copy()), initial_guess=True).clone())
    assert torch.equal(y, y0) and torch.equal(z, z0)
    assert torch.isfinite(y).all() and torch.isfinite(z).all() and float(y.abs().max()) > 0.0


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (3, "km_metric"), (2, "km_packed12"), (1, "curl_metric"), (2, "mass_packed")])
def test_one_bent_edge_keeps_the_general_form(bent, monkeypatch, p, form):
    """A batch with per-point data: the flag is off, the general form runs (switching has no effect) and is correct."""
    op = _apply_checks(bent, p, form, monkeypatch, False)
    col, aff = op.stream_column(), op.stream_affine()
    assert 0 < col[2] + aff[2] < 60  # (the other batches stay compact in the general kernel)


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (3, "km_metric"), (2, "km_packed12"), (1, "km_metric"), (1, "mass_packed"),
                                    (2, "curl_metric")])
def test_element_count_not_a_multiple_of_four(extruded15, monkeypatch, p, form):
    """15 elements: the pad entry of the last batch takes the kind of the three elements it sits with, so the batch -- and with it
    the whole mesh -- stays compact.  The pad entry's rows of both tables lie inside them (they are sized for the padded element
    count; the 64 bytes behind the column table are what the general form's second request of a component may touch, the compact
    form's last request ends at the table's last row) and are zero; its x reads as zero and its results go to E-vector rows nobody
    gathers.  The reports count real elements only."""
    op = _apply_checks(extruded15, p, form, monkeypatch, True)
    col, aff = op.stream_column(), op.stream_affine()
    assert col[0] == 15 and col[2] + aff[2] == 15


@pytest.mark.parametrize("p,form", [(3, "curl_packed"), (3, "km_metric"), (2, "km_packed12"), (1, "mass_packed")])
def test_rotated_elements_keep_the_general_form(rotated, monkeypatch, p, form):
    """Separability along local xi or eta is not looked for: most outer-block elements keep their per-point data."""
    op = _apply_checks(rotated, p, form, monkeypatch, False)
    assert op.stream_column()[1] < 60


def test_forms_off_at_set_up(extruded, monkeypatch):
    """PALACE_AMD_STREAM_COLUMN=0 when the tables are built: the outer blocks' batches read per-point data, no compact form."""
    monkeypatch.setenv("PALACE_AMD_STREAM_COLUMN", "0")
    geom, op, qf, blob = _operator(extruded, 2, "km_packed12", monkeypatch)
    assert op.stream_column() == (60, 0, 0) and not op.stream_compact()
    monkeypatch.delenv("PALACE_AMD_STREAM_COLUMN")
    # with the affine form off every batch is a column batch (an affine element is column-separable by construction)
    monkeypatch.setenv("PALACE_AMD_STREAM_AFFINE", "0")
    M = extruded
    geom1, op1, qf, blob = _operator(M, 2, "km_packed12", monkeypatch)
    assert op1.stream_affine()[2] == 0 and op1.stream_column()[2] == 60 and op1.stream_compact()
    x = np.random.default_rng(5).uniform(-1, 1, M.spaces[2].ndofs)
    y, y0 = _on_off(monkeypatch, lambda: op1.mult(_dev(x), torch.empty(x.size, dtype=torch.float64, device="cuda")).clone())
    assert torch.equal(y, y0)
    assert _rel(y.cpu().numpy(), M.oracle(2, qf, blob, x, "affine-off")) < RTOL
