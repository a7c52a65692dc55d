"""Nonconforming (hanging-node) hexahedral meshes and their constrained H(curl) / H1 / H(div) spaces: the host stand-in for what
the reference gets from MFEM's NCMesh when `Refinement.Nonconformal` is on (utils/geodata.cpp:174-186: tensor elements are only
ever refined this way; `MaxNCLevels = 1`, utils/configfile.hpp:111-116) -- local refinement of hex27 elements, the
master / slave faces and edges of the one-irregular result, the conforming prolongation P = [I; C] of an NDHexSpace or
H1HexSpace on it (every ParOperator of the reference is then P^T A P, linalg/rap.cpp:65, :212-216) and the Doerfler marking of
utils/dorfler.cpp on one rank.

The mesh is held flat: an NCHexMesh lists its leaf elements like any HexMesh, and the topology of HexMesh (vertices, edges and
faces keyed by their corner vertices) then numbers a coarse face and the four fine faces on it as five different faces.  A
face or edge whose tri-quadratic mid node is a vertex of the mesh is a MASTER; the four sub-faces / two sub-edges on it, and the
four cross edges interior to a master face, are its SLAVES.  The space of the wrapped class on this topology is the broken
(partially conforming) space; the dofs on slave entities (and, for H1, the hanging vertices) are constrained: each is the
master element's trace evaluated at the slave's node.  On the shared entity the two elements' reference coordinates differ by
an affine map with factor 1/2 that is read off the node ids (a slave's corners are lattice nodes of the master element), so no
face-frame class has to be enumerated: along the tangent of a covariant dof the open basis on the half interval scaled by
1/2, along every other direction the closed basis on the half interval -- the 1-D matrices of htransfer.hex_child_matrices.
A Raviart-Thomas space (RTHexSpace) has dofs on faces and interiors only, so just the p^2 normal-flux dofs of a slave face are
constrained: the master's normal flux density at the slave node (closed basis along the master's normal, open along the two
tangents) times the determinant +-1/4 of the map between the two reference faces, the contravariant Piola factor.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .basis1d import gauss_legendre, gauss_lobatto
from .fespace import _VERT_IJK, H1HexSpace, NDHexSpace
from .htransfer import hex_child_matrices
from .mesh import _CORNER_LATTICE, HEX_EDGES, HEX_FACE_AXES, HEX_FACES_UV, HexMesh, _merge_points, _q2_1d
from .rthex import RTHexSpace

# lattice index of the mid node of every local edge / face, and of the four edge mid nodes of every local face in the order
# (u at v = 0, u at v = 1, v at u = 0, v at u = 1) of its (c00, c10, c01, c11) corners
_EDGE_MID = (_CORNER_LATTICE[HEX_EDGES[:, 0]] + _CORNER_LATTICE[HEX_EDGES[:, 1]]) // 2
_FACE_MID = _CORNER_LATTICE[HEX_FACES_UV].sum(axis=1) // 4
_FACE_EDGE_MID = np.stack([(_CORNER_LATTICE[HEX_FACES_UV[:, a]] + _CORNER_LATTICE[HEX_FACES_UV[:, b]]) // 2
                           for a, b in ((0, 1), (2, 3), (0, 2), (1, 3))], axis=1)
# the four sub-faces of a master face: (corner, edge mid along u, edge mid along v) as positions in the two lists above
_SUBFACE = ((0, 0, 2), (1, 0, 3), (2, 1, 2), (3, 1, 3))


@dataclass
class NCHexMesh(HexMesh):
    """The leaf elements of a locally refined hex27 mesh.  level [NE]: refinement depth; parent [NE] / child [NE]: the element
    of the mesh this one was refined from that each element is (child -1) or is octant a + 2 b + 4 c of; marked: the closed
    set of elements of that mesh that were split."""
    level: np.ndarray | None = None
    parent: np.ndarray | None = None
    child: np.ndarray | None = None
    marked: np.ndarray | None = None

    def __post_init__(self):
        if self.level is None:
            self.level = np.zeros(self.ne, dtype=np.int32)
        if self.parent is None:
            self.parent, self.child = np.arange(self.ne), np.full(self.ne, -1)
        if self.marked is None:
            self.marked = np.zeros(0, dtype=np.int64)

    def _build_topology(self):
        if "nc" in self._topo:
            return
        super()._build_topology()
        t = self._topo
        nv, verts = t["nv"], t["verts"]
        vert_of = np.full(self.x.shape[0], -1, dtype=np.int64)
        vert_of[t["vert_nodes"]] = np.arange(nv)
        ekeys = t["edge_verts"][:, 0] * nv + t["edge_verts"][:, 1]
        fv = t["face_verts"]
        fkeys = (fv[:, 0] * nv + fv[:, 1]) * nv + fv[:, 2]

        def find(keys, k, what):
            i = np.searchsorted(keys, k)
            if i >= keys.size or keys[i] != k:
                raise ValueError(f"hanging {what} without its slave: the mesh is not one-irregular")
            return int(i)

        def edge_id(a, b):
            return find(ekeys, min(a, b) * nv + max(a, b), "edge")

        def face_id(vs):
            s = sorted(vs)
            return find(fkeys, (s[0] * nv + s[1]) * nv + s[2], "face")

        edge_master = np.full(t["nedges"], -1, dtype=np.int64)   # master EDGE of a sub-edge
        edge_mface = np.full(t["nedges"], -1, dtype=np.int64)    # master FACE of a cross edge
        face_master = np.full(t["nfaces"], -1, dtype=np.int64)
        medges, mfaces = {}, {}                                  # master id -> (element, local entity) that holds it whole
        emid = vert_of[self.elem_nodes[:, _EDGE_MID]]            # [NE, 12] vertex at the edge's mid node, or -1
        for e, le in zip(*np.nonzero(emid >= 0)):
            g = int(t["elem_edges"][e, le])
            if g in medges:
                continue
            medges[g] = (int(e), int(le))
            for v in verts[e, HEX_EDGES[le]]:
                edge_master[edge_id(int(v), int(emid[e, le]))] = g
        fmid = vert_of[self.elem_nodes[:, _FACE_MID]]
        for e, lf in zip(*np.nonzero(fmid >= 0)):
            g = int(t["elem_faces"][e, lf])
            mfaces[g] = (int(e), int(lf))
            m = int(fmid[e, lf])
            mids = [int(v) for v in vert_of[self.elem_nodes[e, _FACE_EDGE_MID[lf]]]]
            if min(mids) < 0:
                raise ValueError("master face with a conforming edge: the mesh is not one-irregular")
            for c, iu, iv in _SUBFACE:
                face_master[face_id([int(verts[e, HEX_FACES_UV[lf, c]]), mids[iu], mids[iv], m])] = g
            for v in mids:
                edge_mface[edge_id(v, m)] = g
        # any element that holds an edge / the element of a face (slaves have exactly one)
        edge_elem = np.zeros((t["nedges"], 2), dtype=np.int64)
        edge_elem[t["elem_edges"].ravel()] = np.stack(np.divmod(np.arange(self.ne * 12), 12), axis=1)
        face_elem = np.zeros((t["nfaces"], 2), dtype=np.int64)
        face_elem[t["elem_faces"].ravel()] = np.stack(np.divmod(np.arange(self.ne * 6), 6), axis=1)
        t["nc"] = dict(edge_master=edge_master, edge_mface=edge_mface, face_master=face_master, medges=medges, mfaces=mfaces,
                       edge_elem=edge_elem, face_elem=face_elem, vert_of=vert_of)

    def _nc(self):
        self._build_topology()
        return self._topo["nc"]

    @property
    def master_faces(self):
        return np.array(sorted(self._nc()["mfaces"]), dtype=np.int64)

    @property
    def master_edges(self):
        return np.array(sorted(self._nc()["medges"]), dtype=np.int64)

    @property
    def slave_faces(self):
        return np.nonzero(self._nc()["face_master"] >= 0)[0]

    @property
    def slave_edges(self):
        """Sub-edges of master edges and the cross edges interior to master faces."""
        nc = self._nc()
        return np.nonzero((nc["edge_master"] >= 0) | (nc["edge_mface"] >= 0))[0]

    @property
    def cross_edges(self):
        return np.nonzero(self._nc()["edge_mface"] >= 0)[0]

    @property
    def hanging_verts(self):
        """Vertices at the mid node of a master edge or face."""
        nc, out = self._nc(), []
        for g, (e, le) in nc["medges"].items():
            out.append(nc["vert_of"][self.elem_nodes[e, _EDGE_MID[le]]])
        for g, (e, lf) in nc["mfaces"].items():
            out.append(nc["vert_of"][self.elem_nodes[e, _FACE_MID[lf]]])
        return np.unique(np.array(out, dtype=np.int64))

    @property
    def boundary_face_mask(self):
        """[nfaces] bool: faces with a single adjacent element that are neither masters nor slaves (both have one adjacent
        element in the flat topology and lie inside the domain)."""
        nc = self._nc()
        mask = self._topo["face_count"] == 1
        mask[nc["face_master"] >= 0] = False
        mask[self.master_faces] = False
        return mask

    def check(self):
        """Q2 node count with hanging nodes: the mid node of a master edge / face is counted among the vertices already."""
        nc = self._nc()
        expect = self.nv + self.nedges + self.nfaces + self.ne - len(nc["medges"]) - len(nc["mfaces"])
        if np.unique(self.elem_nodes).size != expect:
            raise ValueError(f"node merge failed: {np.unique(self.elem_nodes).size} nodes, expected {expect}")
        J = self.jacobian_at(np.array([[0.5, 0.5, 0.5]]))
        if not np.all(np.linalg.det(J[:, 0]) > 0):
            raise ValueError("inverted element")


def _close_marked(mesh, level, marked):
    """One-irregular closure: an element to be split drags along every coarser leaf it shares (part of) an edge with -- the
    element's edge then has both end points among the 27 lattice nodes of the coarser one."""
    import scipy.sparse as sp

    ne, nn = mesh.ne, mesh.x.shape[0]
    inc = sp.csr_matrix((np.ones(ne * 27), (np.repeat(np.arange(ne), 27), mesh.elem_nodes.ravel())), shape=(ne, nn))
    ends = mesh.elem_nodes[:, _CORNER_LATTICE][:, HEX_EDGES]  # [NE, 12, 2] node ids
    marked = marked.copy()
    front = np.nonzero(marked)[0]
    while front.size:
        rows = np.repeat(np.arange(front.size * 12), 2)
        a = sp.csr_matrix((np.ones(rows.size), (rows, ends[front].ravel())), shape=(front.size * 12, nn))
        hit = (a @ inc.T).tocoo()
        both = hit.data > 1.5
        k, n = front[hit.row[both] // 12], hit.col[both]
        new = np.unique(n[(level[n] < level[k]) & ~marked[n]])
        marked[new] = True
        front = new
    return marked


def refine_local(mesh: HexMesh, marked) -> NCHexMesh:
    """Split the marked hex27 elements of a HexMesh or NCHexMesh into 8 (new nodes from the parent's tri-quadratic map, the
    children in the octant order of mesh.refine_uniform), keep the others.  The marked set is first closed so that the result
    is one-irregular: across faces and across edges the refinement level differs by at most 1 (MaxNCLevels = 1).  The closed
    set and every element's parent are the result's `marked`, `parent` and `child`."""
    ne = mesh.ne
    level = getattr(mesh, "level", None)
    level = np.zeros(ne, dtype=np.int32) if level is None else np.asarray(level)
    sel = np.zeros(ne, dtype=bool)
    sel[np.asarray(marked, dtype=np.int64)] = True
    sel = _close_marked(mesh, level, sel)
    t = np.linspace(0.0, 1.0, 5)
    B, _ = _q2_1d(t)
    mk = np.nonzero(sel)[0]
    X = mesh.elem_coords()
    fine = np.einsum("ck,bj,ai,ekjid->ecbad", B, B, B, X[mk].reshape(mk.size, 3, 3, 3, 3))
    kids = np.stack([fine[:, 2 * c:2 * c + 3, 2 * b:2 * b + 3, 2 * a:2 * a + 3, :].reshape(mk.size, 27, 3)
                     for c in range(2) for b in range(2) for a in range(2)], axis=1)  # [nmk, 8, 27, 3]
    count = np.where(sel, 8, 1)
    first = np.concatenate([[0], np.cumsum(count)])
    ne_new = int(first[-1])
    pts = np.empty((ne_new, 27, 3))
    parent = np.repeat(np.arange(ne), count)
    child = np.full(ne_new, -1)
    keep = np.nonzero(~sel)[0]
    pts[first[keep]] = X[keep]
    kid_pos = first[mk][:, None] + np.arange(8)[None, :]
    pts[kid_pos] = kids
    child[kid_pos] = np.arange(8)[None, :]
    lo, hi = mesh.bounding_box()
    upts, inv = _merge_points(pts.reshape(-1, 3), 1e-6 * float(np.max(hi - lo)))
    out = NCHexMesh(x=upts, elem_nodes=inv.reshape(ne_new, 27), attr=mesh.attr[parent],
                    level=(level[parent] + (child >= 0)).astype(np.int32), parent=parent, child=child, marked=mk)
    out.check()
    return out


# ---- constrained spaces --------------------------------------------------------------------

def _lagrange(nodes, x):
    """B[q, i] = l_i(x_q) of the Lagrange basis on `nodes`."""
    d = x[:, None, None] - nodes[None, None, :]                       # [q, i, m]
    w = nodes[:, None] - nodes[None, :]
    n = nodes.size
    eye = np.eye(n, dtype=bool)
    d = np.where(eye[None], 1.0, d)
    w = np.where(eye, 1.0, w)
    return d.prod(axis=2) / w.prod(axis=1)[None, :]


class _NCSpaceMixin:
    """An NDHexSpace / H1HexSpace / RTHexSpace on an NCHexMesh, renumbered so that its true dofs come first and its constrained
    dofs last (the layout of pa_halo_create: true dofs [0, n_true), then the rest), with the conforming prolongation P = [I; C].

    elem_dof_lex (and elem_sign_lex), ndofs = n_local, n_true, C [n_local - n_true, n_true] (scipy CSR), ess_dofs() as true-dof
    indices on the corrected boundary mask, broken_perm [n_local]: the wrapped space's dof d is dof broken_perm[d] here."""

    def _constrain(self):
        import scipy.sparse as sp

        mesh, p = self.mesh, self.p
        hcurl, hdiv = isinstance(self, NDHexSpace), isinstance(self, RTHexSpace)
        nc = mesh._nc() if isinstance(mesh, NCHexMesh) else None
        cp = gauss_lobatto(p + 1)
        op = gauss_legendre(p)[0] if hcurl or hdiv else None
        # reference position and direction of every local dof
        if hcurl or hdiv:
            xi, comp = [], []
            for c in range(3):
                nodes = [op, op, op] if hdiv else [cp, cp, cp]
                nodes[c] = cp if hdiv else op
                K, J, I = np.meshgrid(np.arange(nodes[2].size), np.arange(nodes[1].size), np.arange(nodes[0].size), indexing="ij")
                xi.append(np.stack([nodes[0][I.ravel()], nodes[1][J.ravel()], nodes[2][K.ravel()]], axis=1))
                comp.append(np.full(I.size, c))
            xi, comp = np.concatenate(xi), np.concatenate(comp)
        else:
            K, J, I = np.meshgrid(np.arange(p + 1), np.arange(p + 1), np.arange(p + 1), indexing="ij")
            xi, comp = np.stack([cp[I.ravel()], cp[J.ravel()], cp[K.ravel()]], axis=1), None
        sign = self.elem_sign_lex.astype(np.float64) if hcurl or hdiv else None
        rows = {}  # constrained (broken) dof -> (columns, values)

        def trace_rows(M, S, axes, origin, ldofs):
            """Rows of the dofs `ldofs` of element S, which lie on an entity of S spanned by the reference axes `axes` from
            the corner `origin` (lattice triple), as combinations of element M's dofs."""
            lat_m = {int(n): l for l, n in enumerate(mesh.elem_nodes[M])}

            def at(ijk):  # master reference coordinates of a lattice node of S
                l = lat_m[int(mesh.elem_nodes[S, ijk[0] + 3 * ijk[1] + 9 * ijk[2]])]
                return 0.5 * np.array([l % 3, (l // 3) % 3, l // 9])

            o = at(origin)
            A = np.zeros((3, 3))
            for ax in axes:
                far = list(origin)
                far[ax] = 2
                A[:, ax] = at(far) - o
            xm = o[None, :] + xi[ldofs][:, list(axes)] @ A[:, list(axes)].T
            Bc = [_lagrange(cp, xm[:, d]) for d in range(3)]
            if hcurl:
                Bo = [_lagrange(op, xm[:, d]) for d in range(3)]
                tan = A[:, comp[ldofs]].T                                  # [n, 3] the dof's tangent in M's coordinates
                blocks = []
                for c in range(3):
                    f = [Bo[d] if d == c else Bc[d] for d in range(3)]
                    blocks.append(tan[:, c, None] * np.einsum("nk,nj,ni->nkji", f[2], f[1], f[0]).reshape(len(ldofs), -1))
                R = np.concatenate(blocks, axis=1) * sign[M][None, :] * sign[S, ldofs][:, None]
            elif hdiv:
                # normal flux density of M's field on the face: block mn of M (closed along its normal mn, open along the
                # two tangents) times the contravariant Piola factor det(A_face) = +-1/4 between the two reference faces,
                # both taken with ascending-axis tangents, and the sign e_u x e_v = eps e_n of either reference normal
                uax, vax = axes
                tm = [d for d in range(3) if np.any(A[d] != 0.0)]
                mn = 3 - sum(tm)
                det = np.linalg.det(A[np.ix_(tm, [uax, vax])]) * (-1.0 if uax > vax else 1.0)
                eps = (-1.0 if mn == 1 else 1.0) * (-1.0 if 3 - uax - vax == 1 else 1.0)
                f = [Bc[d] if d == mn else _lagrange(op, xm[:, d]) for d in range(3)]
                R = np.zeros((len(ldofs), self.P))
                nblk = p * p * (p + 1)
                R[:, mn * nblk:(mn + 1) * nblk] = eps * det * np.einsum("nk,nj,ni->nkji", f[2], f[1], f[0]).reshape(len(ldofs), -1)
                R = R * sign[M][None, :] * sign[S, ldofs][:, None]
            else:
                R = np.einsum("nk,nj,ni->nkji", Bc[2], Bc[1], Bc[0]).reshape(len(ldofs), -1)
            gm = self.elem_dof_lex[M]
            for r, l in zip(R, ldofs):
                g = int(self.elem_dof_lex[S, l])
                nz = np.nonzero(np.abs(r) > 1e-13)[0]
                if nz.size == 1 and gm[nz[0]] == g:
                    continue                                               # a dof the two elements share: not constrained
                if g in rows:
                    # the same dof seen from another slave element or through a master edge's other element
                    ref = dict(zip(*rows[g]))
                    assert set(ref) == {int(c) for c in gm[nz]} and all(abs(ref[int(c)] - v) < 1e-12 for c, v in zip(gm[nz], r[nz]))
                    continue
                rows[g] = (gm[nz].astype(np.int64), r[nz])

        if nc is not None:
            on = lambda ax, s: np.abs(xi[:, ax] - s) < 1e-14  # noqa: E731
            for f in np.nonzero(nc["face_master"] >= 0)[0]:
                M, _ = nc["mfaces"][int(nc["face_master"][f])]
                S, lf = nc["face_elem"][f]
                nax, side, uax, vax = HEX_FACE_AXES[lf]
                sel = on(nax, side) & ((comp != nax) if hcurl else (comp == nax) if hdiv else True)
                origin = [0, 0, 0]
                origin[nax] = 2 * side
                trace_rows(M, int(S), (uax, vax), origin, np.nonzero(sel)[0])
            for e in np.nonzero(nc["edge_master"] >= 0)[0] if not hdiv else ():
                M, _ = nc["medges"][int(nc["edge_master"][e])]
                S, le = nc["edge_elem"][e]
                a, b = HEX_EDGES[le]
                ax = int(np.argmax(_VERT_IJK[b] - _VERT_IJK[a]))
                sel = np.ones(xi.shape[0], dtype=bool)
                for d in range(3):
                    if d != ax:
                        sel &= on(d, _VERT_IJK[a][d])
                if hcurl:
                    sel &= comp == ax
                trace_rows(M, int(S), (ax,), list(2 * _VERT_IJK[a]), np.nonzero(sel)[0])
        n_local = self.ndofs
        con = np.zeros(n_local, dtype=bool)
        con[list(rows)] = True
        perm = np.empty(n_local, dtype=np.int64)
        n_true = int(n_local - con.sum())
        perm[~con] = np.arange(n_true)
        perm[con] = n_true + np.arange(n_local - n_true)
        ri, ci, vv = [], [], []
        for g, (cols, vals) in rows.items():
            # one-irregular: no chains, every column is a true dof
            assert not con[cols].any(), "constraint chain: the mesh is not one-irregular"
            ri.append(np.full(cols.size, perm[g] - n_true))
            ci.append(perm[cols])
            vv.append(vals)
        cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dtype=dt)  # noqa: E731
        self.C = sp.csr_matrix((cat(vv, np.float64), (cat(ri, np.int64), cat(ci, np.int64))), shape=(n_local - n_true, n_true))
        self.C.sort_indices()
        self.n_true, self.n_local, self.broken_perm = n_true, n_local, perm
        self.elem_dof_lex = perm[self.elem_dof_lex].astype(np.int32)

    def prolongation(self):
        """P = [I; C] as a scipy CSR matrix [n_local, n_true]."""
        import scipy.sparse as sp

        return sp.vstack([sp.identity(self.n_true, format="csr"), self.C]).tocsr()

    def ess_dofs(self, *args, **kw):
        """Sorted true dofs on the boundary (constrained boundary dofs follow from them: their masters lie on the boundary)."""
        d = super().ess_dofs(*args, **kw)
        return d[d < self.n_true]


class NCNDHexSpace(_NCSpaceMixin, NDHexSpace):
    pass


class NCH1HexSpace(_NCSpaceMixin, H1HexSpace):
    pass


class NCRTHexSpace(_NCSpaceMixin, RTHexSpace):
    """Only the p^2 normal-flux dofs of a slave face are constrained; RT has no edge or vertex dofs and no essential dofs."""

    def ess_dofs(self, *args, **kw):
        return np.zeros(0, dtype=np.int64)


def NCSpace(space):
    """The constrained form of an NDHexSpace, H1HexSpace or RTHexSpace (orders 1 to 5) built on an NCHexMesh; a conforming
    mesh gives a space with zero constraints."""
    cls = NCNDHexSpace if isinstance(space, NDHexSpace) else NCRTHexSpace if isinstance(space, RTHexSpace) else NCH1HexSpace
    assert isinstance(space, (NDHexSpace, H1HexSpace, RTHexSpace)) and not isinstance(space, _NCSpaceMixin)
    out = cls.__new__(cls)
    out.__dict__.update(space.__dict__)
    out.broken = space
    out._constrain()
    return out


def refinement_transfer(coarse, fine):
    """T [fine.ndofs, coarse.ndofs] (scipy CSR) between the spaces of one kind and order on a mesh and on refine_local of it
    (local vectors of either the broken or the constrained numbering): identity on the kept elements, the child matrices of
    htransfer.hex_child_matrices on the split ones.  For a coarse vector in the range of the coarse P every element that
    holds a fine dof gives it the same value; one copy is kept."""
    import scipy.sparse as sp

    fm = fine.mesh
    assert coarse.p == fine.p and fm.parent.size == fm.ne and fm.parent.max() < coarse.mesh.ne
    hcurl = hasattr(coarse, "elem_sign_lex")
    Mk = hex_child_matrices(coarse.p, hcurl)
    P = coarse.P
    mats = np.where((fm.child >= 0)[:, None, None], Mk[np.maximum(fm.child, 0)], np.eye(P)[None])  # [ne_f, P, P]
    if hcurl:
        mats = mats * fine.elem_sign_lex[:, :, None] * coarse.elem_sign_lex[fm.parent][:, None, :]
    r = np.broadcast_to(fine.elem_dof_lex[:, :, None], mats.shape).ravel().astype(np.int64)
    c = np.broadcast_to(coarse.elem_dof_lex[fm.parent][:, None, :], mats.shape).ravel().astype(np.int64)
    v = mats.ravel()
    nz = np.abs(v) > 1e-14
    r, c, v = r[nz], c[nz], v[nz]
    # one element per fine dof: the first that holds it
    owner = np.full(fine.ndofs, -1, dtype=np.int64)
    el = np.repeat(np.arange(fm.ne), P)
    fd = fine.elem_dof_lex.ravel()
    owner[fd[::-1]] = el[::-1]
    e_of = np.broadcast_to(np.arange(fm.ne)[:, None, None], mats.shape).ravel()[nz]
    keep = owner[r] == e_of
    return sp.csr_matrix((v[keep], (r[keep], c[keep])), shape=(fine.ndofs, coarse.ndofs))


def coarse_node_values(coarse, fine, u):
    """The dofs of `coarse` of the function that the local vector u of `fine` represents: the function evaluated at the
    coarse mesh's dof nodes (the nodal interpolant; a left inverse of refinement_transfer).  On a kept element the dofs
    are the fine element's own; on a split one a coarse node lies in the child of its octant, where the child's tensor basis
    is evaluated at the node's child coordinates (a covariant dof times 2: the coarse tangent is twice as long).  A node on
    the interface of two children takes the lower one: the tangential trace is the same from both sides (an open node at 1/2
    -- odd orders -- would not be; orders with one are refused).  Returns a local vector of `coarse`."""
    fm, p = fine.mesh, coarse.p
    hcurl = hasattr(coarse, "elem_sign_lex")
    cp = gauss_lobatto(p + 1)
    op = gauss_legendre(p)[0] if hcurl else None
    assert not hcurl or not np.any(np.abs(op - 0.5) < 1e-12), "an open node on the children's interface"
    # reference node (and direction) of every local dof
    blocks = []
    for c in range(3 if hcurl else 1):
        nodes = [cp, cp, cp]
        if hcurl:
            nodes[c] = op
        K, J, I = np.meshgrid(*[np.arange(nodes[d].size) for d in (2, 1, 0)], indexing="ij")
        blocks.append((c, np.stack([nodes[0][I.ravel()], nodes[1][J.ravel()], nodes[2][K.ravel()]], axis=1)))
    xi = np.concatenate([b[1] for b in blocks])
    comp = np.concatenate([np.full(b[1].shape[0], b[0]) for b in blocks])
    half = (xi > 0.5 + 1e-12).astype(np.int64)
    octant = half[:, 0] + 2 * half[:, 1] + 4 * half[:, 2]
    loc = 2.0 * xi - half                                            # child coordinates of the coarse node
    Bc = [_lagrange(cp, loc[:, d]) for d in range(3)]
    P = coarse.P
    R = np.zeros((P, P))
    if hcurl:
        Bo = [_lagrange(op, loc[:, d]) for d in range(3)]
        n = P // 3
        for c in range(3):
            f = [Bo[d] if d == c else Bc[d] for d in range(3)]
            blk = 2.0 * np.einsum("nk,nj,ni->nkji", f[2], f[1], f[0]).reshape(P, -1)
            R[comp == c, c * n:(c + 1) * n] = blk[comp == c]
    else:
        R = np.einsum("nk,nj,ni->nkji", Bc[2], Bc[1], Bc[0]).reshape(P, -1)
    # fine element of every (parent, octant); kept elements serve all eight
    ne_c = coarse.mesh.ne
    child_of = np.zeros((ne_c, 8), dtype=np.int64)
    kept = fm.child < 0
    child_of[fm.parent[kept]] = np.nonzero(kept)[0][:, None]
    child_of[fm.parent[~kept], fm.child[~kept]] = np.nonzero(~kept)[0]
    split = np.zeros(ne_c, dtype=bool)
    split[fm.parent[~kept]] = True
    fe = child_of[:, octant]                                          # [ne_c, P] fine element that holds the node
    uf = u[fine.elem_dof_lex]                                         # [ne_f, P]
    if hcurl:
        uf = uf * fine.elem_sign_lex
    vals = np.where(split[:, None], np.einsum("lm,elm->el", R, uf[fe]), uf[fe, np.arange(P)[None, :]])
    if hcurl:
        vals = vals * coarse.elem_sign_lex
    out = np.zeros(coarse.ndofs)
    out[coarse.elem_dof_lex] = vals
    return out


def dorfler_mark(err, fraction):
    """Doerfler marking on one rank (utils/dorfler.cpp:14-170): the smallest set of largest-error elements whose squared
    errors sum to at least `fraction` of the total.  As in the reference the set is cut by a threshold -- the squares are
    summed in ascending order, the pivot is the first element that leaves (1 - fraction) of the total below it, and every
    element at least as large as the pivot is marked -- so elements that tie with the pivot are all marked.  Elements
    without error are never marked.  Returns the sorted element indices."""
    err = np.abs(np.asarray(err, dtype=np.float64))
    assert 0.0 <= fraction <= 1.0
    if err.size == 0 or fraction == 0.0 or not err.any():
        return np.zeros(0, dtype=np.int64)
    est = np.sort(err)
    csum = np.cumsum(est * est)
    pivot = int(np.searchsorted(csum, (1.0 - fraction) * csum[-1], side="left"))
    threshold = est[min(pivot, est.size - 1)]
    return np.nonzero((err >= threshold) & (err > 0.0))[0]
