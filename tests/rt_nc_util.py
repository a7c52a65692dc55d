"""Helpers of the Raviart-Thomas hanging-node tests: the constrained RT spaces on the three meshes of tests/nc_util.py, the local
discrete curl as a scipy matrix and the oracle's local RT operators on a constrained space, each built once per session."""
import numpy as np

from oracle import palace_oracle as po
from palace_amd.fem import nchex, rthex
from tests import nc_util as nu
from tests import rthex_util as ru
from tests import util

_cache = {}


def rt_space(name, p):
    key = ("rt", name, p)
    if key not in _cache:
        _cache[key] = nchex.NCSpace(rthex.RTHexSpace(nu.nc_mesh(name), p))
    return _cache[key]


def local_curl(nd, rt):
    """Discrete curl between the local (L-vector) spaces of one order on one mesh as a scipy CSR matrix [rt.ndofs, nd.ndofs]:
    the element matrix of rthex.hex_curl_matrix through the signed element maps, one copy per row (nc_util.local_gradient
    one space further along the sequence)."""
    import scipy.sparse as sp

    Cel = rthex.hex_curl_matrix(nd.p)
    mats = Cel[None] * rt.elem_sign_lex[:, :, None] * nd.elem_sign_lex[:, None, :]
    r = np.broadcast_to(rt.elem_dof_lex[:, :, None], mats.shape).ravel().astype(np.int64)
    c = np.broadcast_to(nd.elem_dof_lex[:, None, :], mats.shape).ravel().astype(np.int64)
    e = np.broadcast_to(np.arange(nd.mesh.ne)[:, None, None], mats.shape).ravel()
    v = mats.ravel()
    owner = np.full(rt.ndofs, -1, dtype=np.int64)
    owner[rt.elem_dof_lex.ravel()[::-1]] = np.repeat(np.arange(rt.mesh.ne), rt.P)[::-1]
    keep = (owner[r] == e) & (np.abs(v) > 1e-14)
    return sp.csr_matrix((v[keep], (r[keep], c[keep])), shape=(rt.ndofs, nd.ndofs))


def injection(space):
    """R [n_true, n_local]: the first n_true rows of a local vector."""
    import scipy.sparse as sp

    return sp.identity(space.n_local, format="csr")[: space.n_true]


def true_curl(name, p):
    """R_rt C_loc P_nd as a scipy CSR matrix [rt.n_true, nd.n_true], with its two spaces."""
    key = ("curl", name, p)
    if key not in _cache:
        nd, rt = nu.nc_space(name, "nd", p), rt_space(name, p)
        _cache[key] = ((injection(rt) @ local_curl(nd, rt) @ nd.prolongation()).tocsr(), nd, rt)
    return _cache[key]


def oracle_rt_local(rt, form, mass="aniso", q1d=None):
    """CeedOperatorOracle of `form` in ("mass", "divdiv", "divdivmass") on the local vectors of an RT space (the contexts of
    tests/rthex_util.py; the meshes of nc_util carry one attribute)."""
    q1d = rt.p + 1 if q1d is None else q1d
    key = ("orc", id(rt), form, mass, q1d)
    if key not in _cache:
        rint, rdiv = ru.tables(rt.p, q1d)
        _, wts = po.hex_quadrature(q1d)
        g = util.oracle_geom(rt.mesh, q1d)
        cm = ru.mass_ctx(mass)
        args = (rt.ndofs, rt.elem_dof_lex, rt.elem_sign_lex < 0)
        if form == "mass":
            o = po.CeedOperatorOracle(*args, rint, rint, g, po.QF_HDIV, cm)
        elif form == "divdiv":
            o = po.CeedOperatorOracle(*args, rint, rdiv, g, po.QF_L2_1, ru.div_ctx(), qw=wts, deriv_comps=1)
        else:
            o = po.CeedOperatorOracle(*args, rint, rdiv, g, po.QF_L2MASS, cm, ru.div_ctx(), qw=wts, deriv_comps=1)
        _cache[key] = (o, rt)
    return _cache[key][0]


def rt_interpolate(rt, field):
    """The RT nodal interpolant of the physical vector field `field` (x [n, 3] -> [n, 3]) as a local vector: at every dof node
    the contravariant Piola pull-back det(J) J^-1 u of the element's tri-quadratic map, its block's component, times the dof's
    sign.  A dof that several elements hold takes the last one's value (they agree where the normal flux is single-valued)."""
    from palace_amd.fem.basis1d import gauss_legendre, gauss_lobatto
    from palace_amd.fem.mesh import _q2_1d

    p, mesh = rt.p, rt.mesh
    cp, op = gauss_lobatto(p + 1), gauss_legendre(p)[0]
    nblk = p * p * (p + 1)
    vals = np.zeros((mesh.ne, rt.P))
    X = mesh.elem_coords().reshape(mesh.ne, 3, 3, 3, 3)
    for c in range(3):
        nodes = [op, op, op]
        nodes[c] = cp
        K, J, I = np.meshgrid(np.arange(nodes[2].size), np.arange(nodes[1].size), np.arange(nodes[0].size), indexing="ij")
        pts = np.stack([nodes[0][I.ravel()], nodes[1][J.ravel()], nodes[2][K.ravel()]], axis=1)
        B = [_q2_1d(pts[:, d])[0] for d in range(3)]
        x = np.einsum("qk,qj,qi,ekjic->eqc", B[2], B[1], B[0], X)
        Jm = mesh.jacobian_at(pts)
        u = field(x.reshape(-1, 3)).reshape(mesh.ne, -1, 3)
        uh = np.linalg.det(Jm)[..., None] * np.linalg.solve(Jm, u[..., None])[..., 0]
        vals[:, c * nblk:(c + 1) * nblk] = uh[:, :, c]
    out = np.zeros(rt.ndofs)
    out[rt.elem_dof_lex] = vals * rt.elem_sign_lex
    return out
