"""Lifetime of the streaming tables (palace_amd/csrc/pa_internal.hpp: StreamTables, one per StreamForm) across
pa_op_set_essential: the masked form is released and rebuilt, the `all` form of the fused smoother step is dropped and comes back
with the next pa_op_prepare_fused_step.

On a 3 x 3 x 1 mesh: nine elements, so the last batch of the four-element kernels and of the two-element five-point kernel is
padded.  Results are compared bit for bit with an operator that was given its list once.

pa_op_set_essential refuses a list that differs from the one already fused (pa_op_essential_state: a second ParOperator then
takes the unfused path), so the second list of the walk is the first one as another array -- reversed, entries repeated -- which
the C interface accepts and rebuilds the tables for; that a different list is refused and leaves the tables as they were is
checked as well.

What this can and cannot catch: the rebuilt tables hold the same bytes as the released ones, so a table that was wrongly KEPT
would pass unnoticed.  A pointer freed twice, or a table freed and still read (its memory reused by the uploads that follow), shows
as a fault or as different bits; so does a rebuilt form whose counts or pointers were not reset by release()."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from palace_amd import ceed, lib  # noqa: E402
from palace_amd.fem.fespace import H1HexSpace, NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import HexMesh  # noqa: E402
from tests import util  # noqa: E402


class ChebStep(C.Structure):  # pa_cheb_step (include/palace_amd.h)
    _fields_ = [("sd", C.c_double), ("sr", C.c_double), ("dinv", C.c_void_p), ("r0", C.c_void_p), ("e_prev", C.c_void_p),
                ("out", C.c_void_p), ("add", C.c_int32)]


@pytest.fixture(scope="module")
def mesh331():
    """3 x 3 x 1 tri-quadratic hexahedra on a gently warped box (no element is affine)."""
    nx, ny, nz = 3, 3, 1
    gx, gy, gz = np.meshgrid(np.linspace(0, 3, 2 * nx + 1), np.linspace(0, 3, 2 * ny + 1), np.linspace(0, 1, 2 * nz + 1), indexing="ij")
    nid = np.arange(gx.size).reshape(gx.shape)
    x = np.stack([gx + 0.05 * np.sin(gy) * gz, gy + 0.04 * np.sin(1.3 * gx), gz + 0.03 * gx * gy / 9.0], axis=-1).reshape(-1, 3)
    conn = [nid[2 * i:2 * i + 3, 2 * j:2 * j + 3, 2 * k:2 * k + 3].transpose(2, 1, 0).reshape(27)  # lattice order: i fastest
            for k in range(nz) for j in range(ny) for i in range(nx)]
    mesh = HexMesh(x=x, elem_nodes=np.array(conn), attr=(np.arange(nx * ny * nz) % 3 + 1).astype(np.int32))
    mesh.check()
    return mesh


def _operator(mesh, block):
    _, scalar = util.make_ctx("scalar", nattr=3)
    _, aniso = util.make_ctx("aniso", nattr=3)
    if block == "nd2q4":  # H(curl) order 2 at four points per direction
        space, geom = NDHexSpace(mesh, 2), ceed.GeomFactorData(mesh, 4)
        return space, ceed.curlcurlmass_operator(geom, space, scalar, aniso)
    if block == "nd1q5":  # H(curl) order 1 at five points
        space, geom = NDHexSpace(mesh, 1), ceed.GeomFactorData(mesh, 5)
        return space, ceed.curlcurlmass_operator(geom, space, scalar, aniso)
    space, geom = H1HexSpace(mesh, 3), ceed.GeomFactorData(mesh, 4)  # H1 order 3 at four points
    return space, ceed.diffusion_operator(geom, space, aniso)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _three_calls(op, vec):
    """Masked pa_op_mult_essential, pa_op_prepare_fused_step, one pa_op_mult_cheb_step; the two results."""
    L = lib.load()
    n = vec["x"].numel()
    y = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    lib.check(L.pa_op_mult_essential(op.handle, _ptr(vec["x"]), _ptr(y), None))
    available = C.c_int(0)
    lib.check(L.pa_op_prepare_fused_step(op.handle, C.byref(available)))
    assert available.value == 1, "the block has no fused smoother step"
    out = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
    step = ChebStep(0.3, 0.7, vec["dinv"].data_ptr(), vec["r0"].data_ptr(), vec["e_prev"].data_ptr(), out.data_ptr(), 0)
    lib.check(L.pa_op_mult_cheb_step(op.handle, _ptr(vec["x"]), C.byref(step), C.c_int(1), None))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(out).all())
    return y, out


@pytest.mark.parametrize("block", ["nd2q4", "nd1q5", "h1p3q4"])
def test_tables_rebuilt_by_set_essential_match_a_fresh_operator(mesh331, block):
    space, A = _operator(mesh331, block)
    assert mesh331.ne == 9 and A.streams(), "the streaming kernel was not selected"
    n = space.ndofs
    rng = np.random.default_rng(11)
    vec = {k: torch.from_numpy(rng.uniform(0.5 if k == "dinv" else -1.0, 1.0, n)).cuda() for k in ("x", "dinv", "r0", "e_prev")}
    L1 = np.asarray(space.ess_dofs(), dtype=np.int32)
    assert 0 < L1.size < n
    L1b = np.concatenate([L1[::-1], L1[:3]]).astype(np.int32)  # the same list as another array
    L2 = np.arange(1, n, 3, dtype=np.int32)                      # a different one
    assert not np.array_equal(np.unique(L2), np.unique(L1))
    A.set_essential(L1)
    y1, s1 = _three_calls(A, vec)
    # the tables are released and built again under a prepared step
    A.set_essential(L1b)
    y2, s2 = _three_calls(A, vec)
    _, B = _operator(mesh331, block)
    B.set_essential(L1b)
    yb, sb = _three_calls(B, vec)
    assert torch.equal(y2, yb) and torch.equal(s2, sb)
    assert torch.equal(y2, y1) and torch.equal(s2, s1)
    # a different list is refused and leaves the tables alone
    with pytest.raises(lib.PalaceAmdError, match="different essential dof list"):
        A.set_essential(L2)
    y3, s3 = _three_calls(A, vec)
    assert torch.equal(y3, yb) and torch.equal(s3, sb)
    # ... while an operator that only ever saw that list takes it (and computes something else)
    _, D = _operator(mesh331, block)
    D.set_essential(L2)
    yd, sd = _three_calls(D, vec)
    assert not torch.equal(yd, yb) and not torch.equal(sd, sb)
