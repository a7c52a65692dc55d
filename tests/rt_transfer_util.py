"""Shared inputs of the Raviart-Thomas p-prolongation tests (test_rt_transfer_host.py, test_rt_transfer_gpu.py): the element
matrix of RT(pc) -> RT(pf) built from its 1-D blocks, the spaces on the two rotated meshes of tests/rthex_util.py, the
InterpOracle of every pair, unit-coefficient mass oracles on the fine rule and a p-multigrid cycle over them, each built once
per session."""
import numpy as np

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import transfer_util as tu

PAIRS = [(pc, pf) for pf in range(2, 6) for pc in range(1, pf)]
_cache = {}


def interp_1d(pc, pf):
    """(Ic [pf+1][pc+1], Io [pf][pc]): the coarse closed Gauss-Lobatto basis at the fine closed nodes, the coarse open
    Gauss-Legendre basis at the fine open nodes (what linalg.Interp hands to the library)."""
    from palace_amd.fem.basis1d import gauss_legendre, gauss_lobatto, lagrange_eval

    Ic = lagrange_eval(gauss_lobatto(pc + 1), gauss_lobatto(pf + 1))[0]
    Io = lagrange_eval(gauss_legendre(pc)[0], gauss_legendre(pf)[0])[0]
    return np.ascontiguousarray(Ic), np.ascontiguousarray(Io)


def matrix(pc, pf):
    """Dense element matrix [P_f, P_c] in tensor order: component c is Ic along direction c and Io along the other two (the
    mirror image of the Nedelec block), first direction fastest."""
    if ("mat", pc, pf) not in _cache:
        Ic, Io = interp_1d(pc, pf)
        bc, bf = pc * pc * (pc + 1), pf * pf * (pf + 1)
        M = np.zeros((3 * bf, 3 * bc))
        for c in range(3):
            m = [Ic if d == c else Io for d in range(3)]
            M[c * bf:(c + 1) * bf, c * bc:(c + 1) * bc] = np.kron(m[2], np.kron(m[1], m[0]))
        _cache["mat", pc, pf] = M
    return _cache["mat", pc, pf]


def spaces(mesh_kind, pc, pf):
    return ru.space(mesh_kind, pc), ru.space(mesh_kind, pf)


def oracle(mesh_kind, pc, pf):
    if ("orc", mesh_kind, pc, pf) not in _cache:
        c, f = spaces(mesh_kind, pc, pf)
        _cache["orc", mesh_kind, pc, pf] = tu.oracle_of(c, f, matrix(pc, pf))
    return _cache["orc", mesh_kind, pc, pf]


def vectors(mesh_kind, pc, pf):
    """The fixed inputs (x_c, x_f) of the parity tests."""
    c, f = spaces(mesh_kind, pc, pf)
    rng = np.random.default_rng(5000 + 10 * pc + pf)
    return rng.uniform(-1, 1, c.ndofs), rng.uniform(-1, 1, f.ndofs)


def mass_oracle(mesh_kind, p, q1d, mass="aniso"):
    """RT mass of order p on the q1d-point rule: ru.oracle, or with mass="unit" the unit coefficient."""
    if mass != "unit":
        return ru.oracle(mesh_kind, p, q1d, "mass", mass)
    if ("mass1", mesh_kind, p, q1d) not in _cache:
        sp = ru.space(mesh_kind, p)
        rint, _ = ru.tables(p, q1d)
        _cache["mass1", mesh_kind, p, q1d] = po.CeedOperatorOracle(sp.ndofs, sp.elem_dof_lex, sp.elem_sign_lex < 0, rint, rint,
                                                                   ru.ogeom(mesh_kind, q1d), po.QF_HDIV, po.CoeffCtx())
    return _cache["mass1", mesh_kind, p, q1d]


class SparseLevel:
    """A level operator of po.GMGOracle / po.ChebyshevOracle from an assembled oracle operator (no essential dofs)."""

    def __init__(self, op):
        self.M = op.assemble_sparse()
        self.n = self.M.shape[0]
        self._d = self.M.diagonal()

    def mult(self, x):
        return self.M @ x

    def diagonal(self):
        return self._d


def mass_levels(mesh_kind, p, mass="unit"):
    """Levels 1 .. p of the RT mass, every one assembled on the rule of the finest (q1d = p + 1): the Galerkin operators."""
    if ("lev", mesh_kind, p, mass) not in _cache:
        _cache["lev", mesh_kind, p, mass] = [SparseLevel(mass_oracle(mesh_kind, l, p + 1, mass)) for l in range(1, p + 1)]
    return _cache["lev", mesh_kind, p, mass]


def gmg_oracle(levels, P, lambda_max=None, coarse=None):
    """The cycle of the flux projector as the reference configures it (linalg/errorestimator.cpp:67-104): 4th-kind Chebyshev of
    order 2, one pre and one post step, sf_max 1; `coarse` a callable r -> z, by default the exact solve of the coarsest level.
    lambda_max [len - 1]: the estimates of levels 1 .. (None: the oracle's own power iteration)."""
    import scipy.sparse.linalg as spla

    if coarse is None:
        lu = spla.splu(levels[0].M.tocsc())
        coarse = lu.solve
    sm = [None] + [po.ChebyshevOracle(levels[l], 2, lambda_max=None if lambda_max is None else lambda_max[l - 1])
                   for l in range(1, len(levels))]
    none = np.zeros(0, dtype=np.int64)
    return po.GMGOracle(levels, [(p.mult, p.mult_transpose) for p in P], sm, coarse, [none] * len(levels))


def oracle_counts(mesh_kind, p, rel_tol=1e-12):
    """(Jacobi, p-multigrid) PCG iterations on the unit-coefficient RT mass of order p, levels 1 .. p, exact coarse solve."""
    lev = mass_levels(mesh_kind, p)
    P = [oracle(mesh_kind, l, l + 1) for l in range(1, p)]
    A = lev[-1]
    b = A.mult(ru.vector(A.n, 77))
    dinv = 1.0 / A.diagonal()
    _, it_j, _ = po.pcg(A.mult, b, lambda r: dinv * r, rel_tol=rel_tol, max_it=500)
    B = gmg_oracle(lev, P)
    _, it_mg, _ = po.pcg(A.mult, b, B.mult, rel_tol=rel_tol, max_it=500)
    return it_j, it_mg
