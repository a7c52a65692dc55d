"""Shared test helpers: build the oracle's view of a problem from the same descriptors the HIP
library receives (native-ordered oriented restriction, dense tables, geometry data)."""
import numpy as np

from oracle import capi
from oracle import palace_oracle as po
from palace_amd.fem.fespace import NDHexSpace

_dense_cache = {}


def dense_tables(nd: NDHexSpace, q1d):
    key = (nd.p, q1d)
    if key not in _dense_cache:
        _dense_cache[key] = po.nd_hex_dense_tables(nd.p, q1d, nd.dof_map_native())
    return _dense_cache[key]


def oracle_geom(mesh, q1d):
    """geom [NE, 11, Q] through the oracle (mesh-node grad table + geom_33 restatement)."""
    _, wts = po.hex_quadrature(q1d)
    G = po.mesh_q2_grad_table(q1d)
    J = np.einsum("dqn,eni->eqid", G, mesh.elem_coords())  # J[e,q,i,d]
    Jcm = np.transpose(J, (0, 1, 3, 2)).reshape(mesh.ne, -1, 9)
    return po.build_geom_factor_33(mesh.attr.astype(np.float64), wts, Jcm)


def make_ctx(kind, nattr=1):
    """Coefficient contexts used across tests: returns (oracle CoeffCtx, raw blob)."""
    if kind == "identity":
        c = po.CoeffCtx()
    elif kind == "scalar":
        c = po.CoeffCtx(attr_mat=[0] * nattr, mat_coeff=[np.array([2.08])])
    elif kind == "aniso":
        rng = np.random.default_rng(7)
        A = rng.uniform(-1, 1, (3, 3))
        spd = A @ A.T + 2.0 * np.eye(3)
        mats = [spd, np.array([0.7])]
        c = po.CoeffCtx(attr_mat=[i % 2 for i in range(nattr)], mat_coeff=mats, a=1.3)
    elif kind == "nonsym":  # general (non-symmetric) 3x3 material: only the matrix-free D can apply it
        rng = np.random.default_rng(9)
        A = rng.uniform(-1, 1, (3, 3)) + 3.0 * np.eye(3)
        c = po.CoeffCtx(attr_mat=[i % 2 for i in range(nattr)], mat_coeff=[A, np.array([0.7])], a=1.1)
    else:
        raise ValueError(kind)
    return c, c.pack()


QF_MAP = {"hcurlhdiv": (po.QF_HCURLHDIV, None), "hdivhcurl": (po.QF_HDIVHCURL, None),  # numpy oracle only
          "hdiv": (po.QF_HDIV, capi.QF_HDIV), "hcurl": (po.QF_HCURL, capi.QF_HCURL),
          "hdivmass": (po.QF_HDIVMASS, capi.QF_HDIVMASS)}


def oracle_apply_c(nd, geom, qf, blob, x, q1d):
    """y = A x through the C oracle (dense tables, oriented restriction)."""
    off, ori = nd.native_restriction()
    interp, curl = dense_tables(nd, q1d)
    y = np.zeros(nd.ndofs)
    capi.apply_add(off, ori, interp, curl, geom, QF_MAP[qf][1], blob, np.ascontiguousarray(x), y)
    return y


def oracle_operator(nd, geom, qf, ctx, ctx2=None, q1d=None):
    off, ori = nd.native_restriction()
    interp, curl = dense_tables(nd, q1d)
    return po.CeedOperatorOracle(nd.ndofs, off, ori, interp, curl, geom, QF_MAP[qf][0], ctx, ctx2)


class FastParOperatorOracle(po.ParOperatorOracle):
    """ParOperatorOracle whose local apply runs through the C oracle (same restatement, compiled)."""

    def __init__(self, nd, geom, qf, blob, ess, q1d, ctx, ctx2=None, policy=po.DIAG_ONE):
        self.nd, self.geom, self.qf, self.blob, self.q1d = nd, geom, qf, blob, q1d
        self.ess = np.asarray(ess, dtype=np.int64)
        self.policy = policy
        self.n = nd.ndofs
        self._np_op = oracle_operator(nd, geom, qf, ctx, ctx2, q1d)
        self._diag = None

    def mult(self, x):
        tx = x.copy()
        tx[self.ess] = 0.0
        y = oracle_apply_c(self.nd, self.geom, self.qf, self.blob, tx, self.q1d)
        y[self.ess] = x[self.ess] if self.policy == po.DIAG_ONE else 0.0
        return y

    def diagonal(self):
        if self._diag is None:
            d = self._np_op.diagonal()
            d[self.ess] = 1.0 if self.policy == po.DIAG_ONE else 0.0
            self._diag = d
        return self._diag


def h1_hex_interp_lex(pc, pf):
    """Dense [(pf+1)^3, (pc+1)^3] element matrix of the H1 p-prolongation in tensor dof order: the Kronecker product of the
    1-D Lagrange matrices (coarse basis functions at the fine closed nodes), i fastest."""
    cpc, cpf = po.gll_points(pc + 1), po.gll_points(pf + 1)
    I1 = np.array([[po.lagrange(cpc, xf, a)[0] for a in range(pc + 1)] for xf in cpf])
    return np.einsum("kc,jb,ia->kjicba", I1, I1, I1).reshape((pf + 1) ** 3, (pc + 1) ** 3)


def hex_rotations():
    """The 24 proper rotations of the reference cube as permutations of the 27 lattice nodes i + 3 j + 9 k (rotation about
    the centre node): returns (R [24, 3, 3] signed permutation matrices with determinant +1, perm [24, 27]) where the rotated
    element's node at lattice position n' = R (n - 1) + 1 is the original element's node at n: elem_nodes' = elem_nodes[perm]."""
    import itertools

    mats, perms = [], []
    n = np.array([[i, j, k] for k in range(3) for j in range(3) for i in range(3)])  # row l = i + 3 j + 9 k
    for axes in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), dtype=np.int64)
            for r in range(3):
                R[r, axes[r]] = signs[r]
            if round(np.linalg.det(R)) != 1:
                continue
            new = (n - 1) @ R.T + 1
            perm = np.empty(27, dtype=np.int64)
            perm[new[:, 0] + 3 * new[:, 1] + 9 * new[:, 2]] = np.arange(27)
            mats.append(R)
            perms.append(perm)
    assert len(mats) == 24 and len({tuple(q) for q in perms}) == 24
    return np.array(mats), np.array(perms)


def rotate_elements(mesh, rot_ids):
    """The same mesh with element e handed over in its rotation rot_ids[e] (an index into hex_rotations()): same nodes, same
    attributes, the 27 node ids of every element permuted.  Vertices, edges and faces are numbered from the node ids alone, so
    they keep their numbers; only the element's own frame (and with it the order and sign of its interior dofs, the local
    position of every edge and face, and the class (ou, ov, swap) of every face) changes."""
    from palace_amd.fem.mesh import HexMesh

    _, perms = hex_rotations()
    rot_ids = np.broadcast_to(np.asarray(rot_ids, dtype=np.int64), (mesh.ne,))
    nodes = np.take_along_axis(mesh.elem_nodes, perms[rot_ids], axis=1)
    out = HexMesh(x=mesh.x, elem_nodes=nodes, attr=mesh.attr, bdr_faces=mesh.bdr_faces, bdr_attr=mesh.bdr_attr)
    out.check()
    assert out.nv == mesh.nv and np.array_equal(out.edge_verts, mesh.edge_verts) and np.array_equal(out.face_verts, mesh.face_verts)
    return out


def element_runs(elem_dof):
    """Number of maximal runs of consecutive dofs in every element's sorted dof list [NE]: what pack_index / pack_index_wide
    (palace_amd/csrc/pa_stream_host.hpp) count against the capacity of the streaming index."""
    d = np.sort(np.asarray(elem_dof, dtype=np.int64), axis=1)
    return 1 + (np.diff(d, axis=1) != 1).sum(axis=1)


def renumbered(space, perm):
    """The same space with dof d renamed perm[d] (a permutation of range(ndofs)): native_restriction() and ess_dofs() read
    elem_dof_lex and follow; a vector x of the original numbering becomes x' with x'[perm] = x."""
    import copy

    perm = np.asarray(perm)
    assert perm.shape == (space.ndofs,) and np.array_equal(np.sort(perm), np.arange(space.ndofs))
    out = copy.copy(space)
    out.elem_dof_lex = perm[space.elem_dof_lex].astype(np.int32)
    return out


def seeded_rotations(ne, seed):
    """A rotation per element: every one of the 24 as often as ne admits, in a seeded random order."""
    return np.random.default_rng(seed).permutation(np.arange(ne) % 24)


def fragmenting_permutation(space, where, target):
    """A renumbering that breaks the dof runs of an element until the largest run count on the mesh is `target`: single dofs at
    offsets 1, 3, 5, ... (each splits a run in three) are exchanged between two blocks of the natural numbering that lie far
    apart -- where = "interior": the interior blocks of the element with the most runs, e0, and of the element 40 further on
    (exclusive dofs: the direct store of the streaming kernels); where = "faces": the blocks of interior faces of e0 and of faces
    of that other element (shared dofs: the E-vector and the run gather).  Returns (perm, runs per element after it)."""
    mesh = space.mesh
    e0 = int(np.argmax(element_runs(space.elem_dof_lex)))
    e1 = (e0 + 40) % mesh.ne
    if where == "interior":
        n = (space.ndofs - space.int_base) // mesh.ne
        pairs = [(space.int_base + e0 * n, space.int_base + e1 * n)]
    else:
        n = (space.int_base - space.face_base) // mesh.nfaces
        inner = lambda e: [int(f) for f in mesh.elem_faces[e] if not mesh.boundary_face_mask[f]]  # noqa: E731
        theirs = [f for f in inner(e1) if f not in set(mesh.elem_faces[e0])]
        pairs = [(space.face_base + a * n, space.face_base + b * n) for a, b in zip(inner(e0), theirs)]
    perm = np.arange(space.ndofs)
    runs = element_runs(space.elem_dof_lex)
    for a, b in pairs:
        for i in range(1, n - 1, 2):
            if runs.max() >= target:
                break
            trial = perm.copy()
            trial[a + i], trial[b + i] = perm[b + i], perm[a + i]
            r = element_runs(trial[space.elem_dof_lex])
            if r.max() <= target:
                perm, runs = trial, r
    return perm, runs


def nd_interpolate(space, F):
    """Nodal interpolant of a smooth vector field F(x) -> [.., 3] in an NDHexSpace-like space:
    dof = F(x_node) . (J e_c) (covariant Piola), written through the signed element->dof map.
    Returns the local vector (size space.ndofs)."""
    from palace_amd.fem.basis1d import gauss_legendre, gauss_lobatto
    from palace_amd.fem.mesh import _q2_1d

    p, mesh = space.p, space.mesh
    cp, op = gauss_lobatto(p + 1), gauss_legendre(p)[0]
    pts, comps = [], []
    for c in range(3):
        n = [p + 1] * 3
        n[c] = p
        nodes = [cp, cp, cp]
        nodes[c] = op
        for k in range(n[2]):
            for j in range(n[1]):
                for i in range(n[0]):
                    pts.append([nodes[0][i], nodes[1][j], nodes[2][k]])
                    comps.append(c)
    pts, comps = np.array(pts), np.array(comps)
    J = mesh.jacobian_at(pts)  # [e, l, i, d]
    Bx, _ = _q2_1d(pts[:, 0])
    By, _ = _q2_1d(pts[:, 1])
    Bz, _ = _q2_1d(pts[:, 2])
    X = mesh.elem_coords().reshape(mesh.ne, 3, 3, 3, 3)
    xp = np.einsum("lk,lj,li,ekjic->elc", Bz, By, Bx, X)
    t = np.take_along_axis(J, comps[None, :, None, None].repeat(mesh.ne, 0).repeat(3, 2), axis=3)[..., 0]
    val = np.einsum("elc,elc->el", F(xp), t) * space.elem_sign_lex
    out = np.zeros(space.ndofs)
    out[space.elem_dof_lex] = val
    return out


def h1_interpolate(space, f):
    """Nodal interpolant of a scalar function f(x) in an H1HexSpace-like space (local vector)."""
    from palace_amd.fem.basis1d import gauss_lobatto
    from palace_amd.fem.mesh import _q2_1d

    p, mesh = space.p, space.mesh
    cp = gauss_lobatto(p + 1)
    pts = np.array([[cp[i], cp[j], cp[k]] for k in range(p + 1) for j in range(p + 1) for i in range(p + 1)])
    Bx, _ = _q2_1d(pts[:, 0])
    By, _ = _q2_1d(pts[:, 1])
    Bz, _ = _q2_1d(pts[:, 2])
    X = mesh.elem_coords().reshape(mesh.ne, 3, 3, 3, 3)
    xp = np.einsum("lk,lj,li,ekjic->elc", Bz, By, Bx, X)
    out = np.zeros(space.ndofs)
    out[space.elem_dof_lex] = f(xp)
    return out
