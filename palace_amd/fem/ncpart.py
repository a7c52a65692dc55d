"""Rank-local view of a constrained (hanging-node) hexahedral space under an element partition: what rcb.PartitionedSpace is
for a plain space, for an nchex.NCSpace (ND, H1 or RT).

Reference: after a nonconformal refinement every run of the reference is still parallel; the conforming prolongation of a
ParFiniteElementSpace is then ONE parallel matrix, the constraint interpolation composed with the exchange of shared dofs
(linalg/rap.cpp:195-234, utils/geodata.cpp:174-186).  Here that composition is P = [I; C_loc] P_halo on the rank-local vector

    [0, n_true)          owned true dofs (the T-vector)
    [n_true, n_shared)   ghost true dofs, grouped by owner (ascending), each group by global number
    [n_shared, n_local)  constrained dofs of the rank's elements (ascending global number)

Constrained dofs are never communicated: a rank that holds one evaluates it from its own copies of the masters.  A rank
therefore also holds every true dof that appears as a column of one of its constrained rows, whether or not one of its
elements contains it -- the master face or edge may belong to another rank's element (a *dependency-only* ghost).

Ownership: the lowest rank among those whose ELEMENTS contain a true dof, so an owner always holds its dof through an element
and the forward transfers' rule "one owner copy is stored" keeps working.  Every rank builds the same global space and
partition (as rcb.PartitionedSpace does), so the plans need no communication: both sides of a rank pair order their lists by
global dof number, dependency-only holders included."""
from __future__ import annotations

import numpy as np

from .fespace import H1HexSpace, NDHexSpace
from .mesh import HexMesh
from .rthex import RTHexSpace


def _held_true(eg, part, C, n_true, q):
    """(true dofs rank q holds through its elements, those it holds only as columns of its constrained rows, its constrained
    dofs), global numbers, each ascending."""
    mine = np.unique(eg[part == q].ravel())
    true_el, con = mine[mine < n_true], mine[mine >= n_true]
    rows = con - n_true
    cols = np.unique(np.concatenate([C.indices[C.indptr[r]:C.indptr[r + 1]] for r in rows])) if rows.size else np.zeros(0, np.int64)
    dep = np.setdiff1d(cols.astype(np.int64), true_el)
    return true_el.astype(np.int64), dep, con.astype(np.int64)


class _ViewMixin:
    """See PartitionedNCSpace (the instance is also an NDHexSpace / H1HexSpace / RTHexSpace on the rank's sub-mesh, so the
    operator and transfer builders take it as a space)."""

    def prolongation(self):
        """[I; C_loc] as a scipy CSR matrix [n_local, n_shared] on the rank's prefix (the halo is not part of it)."""
        import scipy.sparse as sp

        return sp.vstack([sp.identity(self.n_shared, format="csr"), self.C]).tocsr()

    def ess_dofs(self, *args, **kw):
        """Essential TRUE dofs of the rank: the global list restricted to its owned dofs, local numbers."""
        g = np.asarray(self.space.ess_dofs(*args, **kw), dtype=np.int64)
        l = self._g2l[g]
        return np.sort(l[(l >= 0) & (l < self.n_true)]).astype(np.int32)

    def to_local(self, xg):
        """The rank's local vector of a global local-vector (true dofs, then constrained dofs, of the global space)."""
        return np.asarray(xg)[self.l2g]


def PartitionedNCSpace(space, part, rank: int, world: int):
    """Rank `rank`'s view of the nchex.NCSpace `space` (global: every element) under the element partition `part`.

    owner       [space.n_true] owning rank of every global true dof
    elems       global numbers of the rank's elements (increasing); mesh: the sub-mesh of those elements (for GeomFactorData)
    l2g         [n_local] global dof of local dof, in the three ranges above
    n_true, n_shared, n_local = ndofs; n_dep: how many of the ghosts are dependency-only
    elem_dof_lex / elem_sign_lex: the rank's rows, dofs renumbered
    C           local constraint matrix [n_local - n_shared, n_shared] (scipy CSR; entries of a row in the global row's order)
    nbr, send, recv: the halo plan over the prefix [0, n_shared) (send[k]: owned dofs neighbour nbr[k] holds as ghosts,
                recv[k]: ghosts it owns), both in increasing global dof number
    ess_dofs(), to_local(), prolongation()
    """
    import scipy.sparse as sp

    assert hasattr(space, "C") and hasattr(space, "n_true"), "PartitionedNCSpace needs an nchex.NCSpace"
    base = NDHexSpace if isinstance(space, NDHexSpace) else RTHexSpace if isinstance(space, RTHexSpace) else H1HexSpace
    cls = type("Partitioned" + type(space).__name__, (_ViewMixin, base), {})
    v = cls.__new__(cls)
    rank, world = int(rank), int(world)
    v.space, v.rank, v.world, v.p, v.P = space, rank, world, space.p, space.P
    eg = np.asarray(space.elem_dof_lex, dtype=np.int64)
    part = np.asarray(part)
    assert part.shape[0] == eg.shape[0] and part.min() >= 0 and part.max() < world
    n_true_g, n_glob = int(space.n_true), int(space.ndofs)
    Cg = space.C.tocsr()
    # owner of every global true dof: the lowest rank that has it in an element
    owner = np.full(n_glob, world, dtype=np.int64)
    np.minimum.at(owner, eg.ravel(), np.repeat(part.astype(np.int64), eg.shape[1]))
    v.owner = owner[:n_true_g]
    v.elems = np.nonzero(part == rank)[0]
    held = [_held_true(eg, part, Cg, n_true_g, q) for q in range(world)]
    true_el, dep, con = held[rank]
    true_all = np.concatenate([true_el, dep])
    owned = np.sort(true_all[owner[true_all] == rank])
    ghosts = true_all[owner[true_all] != rank]
    ghosts = ghosts[np.lexsort((ghosts, owner[ghosts]))]
    assert np.all(owner[dep] != rank)  # (an owner holds its dof through an element)
    v.l2g = np.concatenate([owned, ghosts, con]).astype(np.int64)
    v.n_true, v.n_shared, v.ndofs = int(owned.size), int(owned.size + ghosts.size), int(v.l2g.size)
    v.n_local, v.n_dep = v.ndofs, int(dep.size)
    g2l = np.full(n_glob, -1, dtype=np.int64)
    g2l[v.l2g] = np.arange(v.ndofs)
    v._g2l = g2l
    v.elem_dof_lex = g2l[eg[v.elems]].astype(np.int32)
    if hasattr(space, "elem_sign_lex"):
        v.elem_sign_lex = space.elem_sign_lex[v.elems]
    # the rank's rows of C with local column numbers; every column is held (element or dependency-only): < n_shared
    rows = con - n_true_g
    cnt = (Cg.indptr[rows + 1] - Cg.indptr[rows]).astype(np.int64) if rows.size else np.zeros(0, np.int64)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    take = np.concatenate([np.arange(Cg.indptr[r], Cg.indptr[r + 1]) for r in rows]) if rows.size else np.zeros(0, np.int64)
    cols = g2l[Cg.indices[take]]
    assert cols.size == 0 or (cols.min() >= 0 and cols.max() < v.n_shared)
    v.C = sp.csr_matrix((Cg.data[take].astype(np.float64), cols.astype(np.int32), indptr), shape=(con.size, v.n_shared))
    m = space.mesh
    v.mesh = HexMesh(x=m.x, elem_nodes=m.elem_nodes[v.elems], attr=m.attr[v.elems])
    # halo plan: who holds a true dof -- through an element or through a constrained row
    v.nbr, v.send, v.recv = [], [], []
    gh_owner = owner[ghosts]
    for q in range(world):
        if q == rank:
            continue
        theirs = np.concatenate([held[q][0], held[q][1]])
        s = np.sort(theirs[owner[theirs] == rank])   # my owned dofs that q holds as ghosts
        r = ghosts[gh_owner == q]                     # increasing global number within the owner's group
        if s.size == 0 and r.size == 0:
            continue
        v.nbr.append(q)
        v.send.append(g2l[s].astype(np.int32))
        v.recv.append(g2l[r].astype(np.int32))
    return v
