"""The operators between spaces on hexahedra (palace_amd/csrc/pa_interp.hip): the p-prolongation of the ND and H1 families,
the discrete gradient and their transposes against po.InterpOracle, for every specialised instantiation of interp_kernel_s and
for the generic interp_kernel (fine order 5), on the two meshes of tests/rthex_util.py whose elements are handed over in seeded
rotations (negative orientation signs on both sides of the transfer, interior dofs in rotated frames; 15 elements leave a
partial wave or block at every order).  tests/test_hex_instantiations.py checks the lists below against the compiled ones and
the oracle-side facts (equal copies of shared dofs, the commuting diagram) on the CPU."""
import numpy as np
import pytest

from tests import rthex_util as ru
from tests import transfer_util as tu

pytestmark = pytest.mark.gpu

ND_PAIRS = [(1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4), (1, 5), (2, 5), (3, 5), (4, 5)]
H1_PAIRS = list(ND_PAIRS)
GRAD_ORDERS = [1, 2, 3, 4, 5]
CASES = [("nd", pc, pf) for pc, pf in ND_PAIRS] + [("h1", pc, pf) for pc, pf in H1_PAIRS] + [("grad", p, p) for p in GRAD_ORDERS]

REL = 1e-13   # transfers against the oracle, 2-norm (test_solvers_gpu.py::test_prolongation_and_transpose, test_h1_gpu.py)
ADJ = 1e-12   # adjointness (the same test)
_ctx = []


def _context():
    from palace_amd import linalg

    if not _ctx:
        _ctx.append(linalg.Context())
    return _ctx[0]


def _device_operator(c, f, kind, **kw):
    from palace_amd import linalg

    return (linalg.Gradient if kind == "grad" else linalg.Interp)(_context(), c, f, **kw)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    import torch

    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _check_parity(T, o, xc, xf):
    """Forward and transpose against the oracle into NaN-filled outputs, adjointness and repeatability of the device results."""
    import torch

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


@pytest.mark.parametrize("mesh_kind", ru.MESHES)
@pytest.mark.parametrize("kind,pc,pf", CASES)
def test_transfer_parity(mesh_kind, kind, pc, pf):
    c, f = tu.spaces(mesh_kind, kind, pc, pf)
    assert kind == "h1" or ((tu.signs(f) < 0).any() and (kind == "grad" or (tu.signs(c) < 0).any()))
    _check_parity(_device_operator(c, f, kind), tu.oracle(mesh_kind, kind, pc, pf), *tu.vectors(mesh_kind, kind, pc, pf))


@pytest.mark.parametrize("pc,pf", ND_PAIRS)
def test_commuting_diagram_on_the_device(pc, pf):
    """G_f P_h1 phi = P_nd G_c phi: four device operators, no oracle."""
    k = "ogrid15"
    hc, hf, nc, nf = tu.space(k, "h1", pc), tu.space(k, "h1", pf), tu.space(k, "nd", pc), tu.space(k, "nd", pf)
    P_h1, P_nd = _device_operator(hc, hf, "h1"), _device_operator(nc, nf, "nd")
    G_c, G_f = _device_operator(hc, nc, "grad"), _device_operator(hf, nf, "grad")
    phi = _dev(ru.vector(hc.ndofs, 7 + 10 * pc + pf))
    a = G_f.mult(P_h1.mult(phi, _nan(hf.ndofs)), _nan(nf.ndofs)).cpu().numpy()
    b = P_nd.mult(G_c.mult(phi, _nan(nc.ndofs)), _nan(nf.ndofs)).cpu().numpy()
    err = tu.rel(a, b)
    print(f"commuting diagram {err:.2e}")
    assert np.linalg.norm(b) > 0.0 and err < 1e-12


def test_four_dof_gather():
    """The transposed gather takes four dofs per thread (k_gather_t<4>) from 2^18 coarse dofs on: ND (3, 4) on 3 520 elements,
    294 129 coarse dofs, the last block of 1 024 partial."""
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.fem.mesh import cylinder_for_dofs

    mesh = cylinder_for_dofs(2.75e5, 3)
    c, f = NDHexSpace(mesh, 3), NDHexSpace(mesh, 4)
    assert mesh.ne == 3520 and c.ndofs == 294129 and c.ndofs >= 1 << 18 and c.ndofs % 1024 != 0
    o = tu.oracle_of(c, f, tu.matrix("nd", 3, 4))
    P = _device_operator(c, f, "nd")
    rng = np.random.default_rng(34)
    xc, xf = rng.uniform(-1, 1, c.ndofs), rng.uniform(-1, 1, f.ndofs)
    yc = P.mult_transpose(_dev(xf), _nan(c.ndofs)).cpu().numpy()
    yf = P.mult(_dev(xc), _nan(f.ndofs)).cpu().numpy()
    assert not np.isnan(yc).any() and not np.isnan(yf).any()
    e_c, e_f = tu.rel(yc, o.mult_transpose(xf)), tu.rel(yf, o.mult(xc))
    print(f"transpose {e_c:.2e} forward {e_f:.2e}")
    assert e_c < REL
    assert e_f < REL


@pytest.mark.parametrize("kind,pc,pf", [("nd", 2, 3), ("h1", 1, 4), ("grad", 3, 3)])
def test_staging_branch_without_a_halo(kind, pc, pf):
    """Fewer true than local fine dofs on one rank (no halo): the operator runs on its staging vectors.  mult gives the first
    n_true entries of the full operator's result and mult_transpose what the full one gives for the zero-padded input."""
    import torch

    c, f = tu.spaces("ogrid15", kind, pc, pf)
    k = 37
    nt = f.ndofs - k
    full = _device_operator(c, f, kind)
    part = _device_operator(c, f, kind, **{"n_true_nd" if kind == "grad" else "n_true_f": nt})
    xc, xf = tu.vectors("ogrid15", kind, pc, pf)
    yf = full.mult(_dev(xc), _nan(f.ndofs))
    for _ in range(2):  # (the second call finds the staging vectors used)
        assert torch.equal(part.mult(_dev(xc), _nan(nt)), yf[:nt])
    xp = xf.copy()
    xp[nt:] = 0.0
    yc = full.mult_transpose(_dev(xp), _nan(c.ndofs))
    assert not torch.isnan(yc).any() and not torch.isnan(yf).any()
    for _ in range(2):
        assert torch.equal(part.mult_transpose(_dev(xf[:nt]), _nan(c.ndofs)), yc)
    assert tu.rel(yc.cpu().numpy(), tu.oracle("ogrid15", kind, pc, pf).mult_transpose(xp)) < REL
