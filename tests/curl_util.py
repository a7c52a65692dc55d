"""Shared inputs of the discrete-curl tests on hexahedra (test_curl_hex_host.py, test_curl_hex_gpu.py,
test_cxx_curl_hex_gpu.py): the Nedelec / Raviart-Thomas pair of one order on the two rotated meshes of tests/rthex_util.py, the
element matrix built from its 1-D blocks, the InterpOracle of the curl and the bound of the exact-sequence tests, each built
once per session."""
import numpy as np

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import transfer_util as tu

ORDERS = [1, 2, 3, 4, 5]
EPS = 2.2e-16
_cache = {}


def spaces(mesh_kind, p):
    """(Nedelec space, Raviart-Thomas space) of order p on ru.mesh(mesh_kind)."""
    return tu.space(mesh_kind, "nd", p), ru.space(mesh_kind, p)


def matrix(p):
    if ("mat", p) not in _cache:
        from palace_amd.fem import rthex

        _cache["mat", p] = rthex.hex_curl_matrix(p)
    return _cache["mat", p]


def derivative_1d(p):
    """Dg [p][p+1]: derivative of the closed Gauss-Lobatto basis at the open Gauss-Legendre nodes (what linalg.Gradient and
    linalg.Curl hand to the library)."""
    from palace_amd.fem.basis1d import gauss_legendre, gauss_lobatto, lagrange_eval

    return np.ascontiguousarray(lagrange_eval(gauss_lobatto(p + 1), gauss_legendre(p)[0])[1])


def block_matrix(p):
    """The element matrix [P_RT, P_ND] assembled from +- I x Dg x I blocks alone: RT component c is D_d ND_e - D_e ND_d for the
    cyclic triple (c, d, e), each term one 1-D contraction with Dg along the differentiated direction."""
    from palace_amd.fem.fespace import nd_block_shape
    from palace_amd.fem.rthex import rt_block_shape

    Dg = derivative_1d(p)
    n1 = p + 1
    C = np.zeros((3 * p * p * n1, 3 * p * n1 * n1))
    for c in range(3):
        d, e = (c + 1) % 3, (c + 2) % 3
        rs = rt_block_shape(p, c)
        for nc, along, sign in ((e, d, 1.0), (d, e, -1.0)):  # ND component, differentiated direction
            ns = nd_block_shape(p, nc)
            for r in np.ndindex(*rs[::-1]):
                ri = r[::-1]  # (i0, i1, i2)
                row = c * p * p * n1 + ri[0] + rs[0] * (ri[1] + rs[1] * ri[2])
                for a in range(n1):
                    ni = list(ri)
                    ni[along] = a
                    col = nc * p * n1 * n1 + ni[0] + ns[0] * (ni[1] + ns[1] * ni[2])
                    C[row, col] = sign * Dg[ri[along], a]
    return C


def oracle_of(nd, rt, p):
    return po.InterpOracle(nd.elem_dof_lex, nd.elem_sign_lex, rt.elem_dof_lex, rt.elem_sign_lex, nd.ndofs, rt.ndofs, matrix(p))


def oracle(mesh_kind, p):
    if ("orc", mesh_kind, p) not in _cache:
        _cache["orc", mesh_kind, p] = oracle_of(*spaces(mesh_kind, p), p)
    return _cache["orc", mesh_kind, p]


def vectors(mesh_kind, p):
    """The fixed inputs (x_nd, x_rt) of the parity tests."""
    nd, rt = spaces(mesh_kind, p)
    rng = np.random.default_rng(4000 + p)
    return rng.uniform(-1, 1, nd.ndofs), rng.uniform(-1, 1, rt.ndofs)


def exactness_bound(p, g):
    """Bound on max |C g| for a discrete gradient g = G phi: 16 eps max |g| max_i sum_j |C_ij|.  Rows of C are sums of
    2 (p + 1) <= 12 products (a-priori factor 12); the rest is room for the rounding of G phi itself."""
    return 16.0 * EPS * np.abs(g).max() * np.abs(matrix(p)).sum(axis=1).max()
