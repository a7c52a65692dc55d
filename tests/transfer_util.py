"""Shared inputs of the hex transfer tests (test_hex_transfer_gpu.py, test_hex_instantiations.py): the ND and H1 spaces on the
two rotated meshes of tests/rthex_util.py, the dense element matrices and the InterpOracle of every transfer, each built once
per session.  A transfer is named (kind, pc, pf): kind "nd" / "h1" the p-prolongation of that family, "grad" the discrete
gradient H1(p) -> ND(p) with pc = pf = p."""
import numpy as np

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import util

_cache = {}


def space(mesh_kind, family, p):
    """family "nd" / "h1" on ru.mesh(mesh_kind)."""
    if ("space", mesh_kind, family, p) not in _cache:
        from palace_amd.fem.fespace import H1HexSpace, NDHexSpace

        _cache["space", mesh_kind, family, p] = (NDHexSpace if family == "nd" else H1HexSpace)(ru.mesh(mesh_kind), p)
    return _cache["space", mesh_kind, family, p]


def spaces(mesh_kind, kind, pc, pf):
    """(domain space, range space) of the transfer."""
    if kind == "grad":
        return space(mesh_kind, "h1", pf), space(mesh_kind, "nd", pf)
    return space(mesh_kind, kind, pc), space(mesh_kind, kind, pf)


def matrix(kind, pc, pf):
    """Dense element matrix [P_range, P_domain] in tensor dof order."""
    if ("mat", kind, pc, pf) not in _cache:
        if kind == "nd":
            M = po.nd_hex_interp_lex(pc, pf)
        elif kind == "h1":
            M = util.h1_hex_interp_lex(pc, pf)
        else:
            M = po.nd_hex_gradient_lex(pf)
        _cache["mat", kind, pc, pf] = M
    return _cache["mat", kind, pc, pf]


def signs(sp):
    """Orientation signs [ne, P] of a space (H1: all ones)."""
    return sp.elem_sign_lex if hasattr(sp, "elem_sign_lex") else np.ones(sp.elem_dof_lex.shape, dtype=np.int8)


def oracle_of(c, f, M):
    return po.InterpOracle(c.elem_dof_lex, signs(c), f.elem_dof_lex, signs(f), c.ndofs, f.ndofs, M)


def oracle(mesh_kind, kind, pc, pf):
    if ("orc", mesh_kind, kind, pc, pf) not in _cache:
        c, f = spaces(mesh_kind, kind, pc, pf)
        _cache["orc", mesh_kind, kind, pc, pf] = oracle_of(c, f, matrix(kind, pc, pf))
    return _cache["orc", mesh_kind, kind, pc, pf]


def vectors(mesh_kind, kind, pc, pf):
    """The fixed inputs (x_c, x_f) of the parity tests."""
    c, f = spaces(mesh_kind, kind, pc, pf)
    rng = np.random.default_rng(1000 * ("nd", "h1", "grad").index(kind) + 10 * pc + pf)
    return rng.uniform(-1, 1, c.ndofs), rng.uniform(-1, 1, f.ndofs)


def rel(a, ref):
    """Relative distance in the 2-norm."""
    return np.linalg.norm(a - ref) / np.linalg.norm(ref)


def copy_spread(o, x):
    """Largest spread among the copies that the elements sharing a range dof compute for it (the E_f-side values of
    o.mult(x) before they are added and divided by the multiplicity), relative to the largest value."""
    ve = ((x[o.dc] * o.sc) @ o.M.T) * o.sf
    hi, lo = np.full(o.nf, -np.inf), np.full(o.nf, np.inf)
    np.maximum.at(hi, o.df.ravel(), ve.ravel())
    np.minimum.at(lo, o.df.ravel(), ve.ravel())
    return (hi - lo).max() / np.abs(ve).max()


def elems_per_wave(pf):
    """Elements a 64-lane wave of the transfer kernels holds at fine order pf ((pf + 1)^2 lanes each); four waves per block."""
    return 64 // (pf + 1) ** 2
