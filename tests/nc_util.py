"""Helpers of the hanging-node tests: the three locally refined meshes, the oracle's local operators on a constrained space
and a ParOperator oracle with a general (scipy) conforming prolongation."""
import os

import numpy as np

from oracle import palace_oracle as po
from palace_amd.fem import nchex
from palace_amd.fem.fespace import H1HexSpace, NDHexSpace
from palace_amd.fem.mesh import HexMesh, _merge_points
from tests import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def block_mesh(n=2):
    """n x n x n unit-cube hex27 elements, local vertex orders scrambled so that every face-frame class occurs."""
    t = np.arange(2 * n + 1) * 0.5
    K, J, I = np.meshgrid(t, t, t, indexing="ij")
    pts = np.stack([I.ravel(), J.ravel(), K.ravel()], axis=1)
    nid = np.arange(pts.shape[0]).reshape(2 * n + 1, 2 * n + 1, 2 * n + 1)
    conn = [nid[2 * k:2 * k + 3, 2 * j:2 * j + 3, 2 * i:2 * i + 3].ravel() for k in range(n) for j in range(n) for i in range(n)]
    upts, inv = _merge_points(pts, 1e-6)
    mesh = HexMesh(x=upts, elem_nodes=inv[np.array(conn)], attr=np.ones(n**3, dtype=np.int32))
    mesh.check()
    return util.rotate_elements(mesh, util.seeded_rotations(mesh.ne, 5))


def cylinder_mesh():
    z = np.load(os.path.join(GOLDEN, "cylinder_hex_mesh.npz"))
    mesh = HexMesh(x=z["x"], elem_nodes=z["elem_nodes"].astype(np.int64), attr=z["attr"].astype(np.int32))
    mesh.check()
    return mesh


def start_mesh(name):
    key = ("start", name)
    if key not in _cache:
        _cache[key] = cylinder_mesh() if name == "C" else block_mesh()
    return _cache[key]


def cylinder_marked(mesh):
    """A seeded 25 % of the elements."""
    return np.sort(np.random.default_rng(11).permutation(mesh.ne)[: mesh.ne // 4])


def nc_mesh(name):
    """A: element 0 of the block refined.  B: elements 0 and 1 (face neighbours) refined, then one child of each again (the
    closure has to split more).  C: the 80-element curved cylinder with a seeded quarter of its elements refined."""
    key = ("nc", name)
    if key not in _cache:
        m0 = start_mesh(name)
        if name == "A":
            m = nchex.refine_local(m0, [0])
        elif name == "B":
            assert np.intersect1d(m0.elem_faces[0], m0.elem_faces[1]).size == 1
            m1 = nchex.refine_local(m0, [0, 1])
            kids = [int(np.nonzero(m1.parent == e)[0][7 if e == 0 else 0]) for e in (0, 1)]
            m = nchex.refine_local(m1, kids)
            m.first = m1
        else:
            m = nchex.refine_local(m0, cylinder_marked(m0))
        _cache[key] = m
    return _cache[key]


def nc_space(name, kind, p):
    key = ("space", name, kind, p)
    if key not in _cache:
        cls = NDHexSpace if kind == "nd" else H1HexSpace
        _cache[key] = nchex.NCSpace(cls(nc_mesh(name), p))
    return _cache[key]


def shifted(a, off):
    """A device copy of `a` that starts `off` doubles past a fresh allocation (off = 1: not on a 16-byte boundary)."""
    import torch

    buf = torch.zeros(a.size + off, dtype=torch.float64, device="cuda")
    buf[off:] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf[off:]


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def oracle_local(space, qf, ctx, ctx2=None, q1d=None):
    """The oracle's local (L-vector) operator of an NDHexSpace / H1HexSpace-like space: qf in 'hdiv' (curl-curl), 'hcurl'
    (ND mass / H1 diffusion), 'hdivmass' (ND K + M), 'h1mass', 'hcurlmass' (H1 diffusion + mass)."""
    q1d = space.p + 1 if q1d is None else q1d
    geom = util.oracle_geom(space.mesh, q1d)
    if isinstance(space, NDHexSpace):
        return util.oracle_operator(space, geom, qf, ctx, ctx2, q1d)
    interp, grad = po.h1_hex_dense_tables(space.p, q1d)
    name = {"hcurl": po.QF_HCURL, "h1mass": po.QF_H1MASS, "hcurlmass": po.QF_HCURLMASS}[qf]
    return po.CeedOperatorOracle(space.ndofs, space.elem_dof_lex, None, interp, grad, geom, name, ctx, ctx2, vector_fe=False)


class CLocal:
    """The oracle's local K + M on an NDHexSpace-like space with the apply through the C restatement (util.oracle_apply_c,
    what util.FastParOperatorOracle does for a conforming space) and a diagonal that does not form element matrices: the
    oracle's own pointwise functions applied to the three unit vectors give the 3 x 3 matrices at every point, and
    diag(B^T D B)[l] = sum_q b_l(q)^T D(q) b_l(q) (signs square to one)."""

    def __init__(self, nd, blob, q1d, ctx_mass, ctx_curl):
        self.nd, self.blob, self.q1d, self.ctxs = nd, blob, q1d, (ctx_mass, ctx_curl)
        self.geom = util.oracle_geom(nd.mesh, q1d)
        self.np_op = util.oracle_operator(nd, self.geom, "hdivmass", ctx_mass, ctx_curl, q1d)

    def apply_add(self, x, y):
        y += util.oracle_apply_c(self.nd, self.geom, "hdivmass", self.blob, x, self.q1d)
        return y

    def diagonal(self):
        o, g = self.np_op, self.geom
        unit = np.zeros((3,) + (g.shape[0], 3, g.shape[2]))
        for i in range(3):
            unit[i, :, i, :] = 1.0
        Dm = np.stack([po.apply_hcurl_33(self.ctxs[0], g, unit[i]) for i in range(3)], axis=-1)  # [NE, 3, Q, 3]
        Dc = np.stack([po.apply_hdiv_33(self.ctxs[1], g, unit[i]) for i in range(3)], axis=-1)
        de = np.einsum("iql,eiqj,jql->el", o.interp, Dm, o.interp) + np.einsum("iql,eiqj,jql->el", o.deriv, Dc, o.deriv)
        d = np.zeros(o.lsize)
        np.add.at(d, o.off.ravel(), de.ravel())
        return d


class ConstrainedParOperatorOracle:
    """rap.cpp:154-361 with a general conforming prolongation P (scipy sparse [n_local, n_true]): y = P^T A P x with the
    essential rows and columns handled as ParOperator::Mult does, the diagonal |P|^T diag(A) (rap.cpp:163-175).  Duck-typed
    like po.ParOperatorOracle (.mult, .diagonal(), .n), so ChebyshevOracle and GMGOracle take it as it is."""

    def __init__(self, ops, P, ess, diag_policy=po.DIAG_ONE):
        self.ops, self.P = list(ops), P.tocsr()
        self.ess = np.asarray(ess, dtype=np.int64)
        self.policy = diag_policy
        self.n = P.shape[1]

    def _local(self, lx):
        ly = np.zeros(self.P.shape[0])
        for op in self.ops:
            op.apply_add(lx, ly)
        return ly

    def mult(self, x):
        tx = x.copy()
        tx[self.ess] = 0.0
        y = self.P.T @ self._local(self.P @ tx)
        y[self.ess] = x[self.ess] if self.policy == po.DIAG_ONE else 0.0
        return y

    mult_transpose = mult  # symmetric local operators only

    def add_mult(self, x, y, a=1.0):
        return y + a * self.mult(x)

    def eliminate_rhs(self, x, b):
        tx = np.zeros(self.n)
        tx[self.ess] = x[self.ess]
        b = b - self.P.T @ self._local(self.P @ tx)
        b[self.ess] = x[self.ess] if self.policy == po.DIAG_ONE else 0.0
        return b

    def diagonal(self):
        d = np.zeros(self.P.shape[0])
        for op in self.ops:
            d += op.diagonal()
        d = abs(self.P).T @ d
        d[self.ess] = 1.0 if self.policy == po.DIAG_ONE else 0.0
        return d

    def dense(self):
        """P^T A P with the essential handling as a dense matrix."""
        return np.stack([self.mult(e) for e in np.eye(self.n)], axis=1)


def local_gradient(h1, nd):
    """Discrete gradient between the local (L-vector) spaces of one order on one mesh as a scipy CSR matrix [nd.ndofs,
    h1.ndofs]: the element matrix of po.nd_hex_gradient_lex through the signed element maps, one copy per row."""
    import scipy.sparse as sp

    Gel = po.nd_hex_gradient_lex(nd.p)
    mats = Gel[None] * nd.elem_sign_lex[:, :, None]
    r = np.broadcast_to(nd.elem_dof_lex[:, :, None], mats.shape).ravel().astype(np.int64)
    c = np.broadcast_to(h1.elem_dof_lex[:, None, :], mats.shape).ravel().astype(np.int64)
    e = np.broadcast_to(np.arange(nd.mesh.ne)[:, None, None], mats.shape).ravel()
    v = mats.ravel()
    owner = np.full(nd.ndofs, -1, dtype=np.int64)
    owner[nd.elem_dof_lex.ravel()[::-1]] = np.repeat(np.arange(nd.mesh.ne), nd.P)[::-1]
    keep = (owner[r] == e) & (np.abs(v) > 1e-14)
    return sp.csr_matrix((v[keep], (r[keep], c[keep])), shape=(nd.ndofs, h1.ndofs))
