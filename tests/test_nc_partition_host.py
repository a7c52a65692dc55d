"""Rank-local views of a constrained space under an element partition (palace_amd/fem/ncpart.py) against the global scipy P:
the three ranges of the local vector, ownership through elements, dependency-only ghosts, the halo plan, and P / P^T / |P|^T
as [I; C_loc] composed with the exchange.  Host only."""
import numpy as np
import pytest

from palace_amd.fem import nchex, rcb
from palace_amd.fem.fespace import H1HexSpace, NDHexSpace
from palace_amd.fem.ncpart import PartitionedNCSpace
from palace_amd.fem.rthex import RTHexSpace
from tests import nc_util as nu

KINDS = {"nd": NDHexSpace, "h1": H1HexSpace, "rt": RTHexSpace}
_spaces, _views = {}, {}


def _space(name, kind, p):
    key = (name, kind, p)
    if key not in _spaces:
        _spaces[key] = nu.nc_space(name, kind, p) if kind != "rt" else nchex.NCSpace(RTHexSpace(nu.nc_mesh(name), p))
    return _spaces[key]


def _part(name, how):
    """(part, world): 'rcbN' or, on A, 'hand': the eight children on rank 0, the rest on rank 1."""
    mesh = nu.nc_mesh(name)
    if how == "hand":
        return np.where(mesh.child >= 0, 0, 1).astype(np.int32), 2
    world = int(how[3:])
    return rcb.rcb(mesh.elem_coords().mean(axis=1), world), world


def _view_set(name, kind, p, how):
    key = (name, kind, p, how)
    if key not in _views:
        part, world = _part(name, how)
        s = _space(name, kind, p)
        _views[key] = (s, part, [PartitionedNCSpace(s, part, r, world) for r in range(world)])
    return _views[key]


CASES = [(name, kind, p, how) for name in "ABC" for kind in KINDS for p in (1, 2, 3)
         for how in (("rcb2", "rcb3", "rcb4") + (("hand",) if name == "A" else ()))]


def _halo_add(views, t):
    """The halo's P^T on the host through the send / recv lists: ghosts of t[r] are added to their owners' entries."""
    out = [x.copy() for x in t]
    for v in views:
        for k, q in enumerate(v.nbr):
            w = views[q]
            j = w.nbr.index(v.rank)
            out[q][w.send[j]] += t[v.rank][v.recv[k]]
    return out


@pytest.mark.parametrize("name,kind,p,how", CASES)
def test_views_against_global_prolongation(name, kind, p, how):
    s, part, views = _view_set(name, kind, p, how)
    world = len(views)
    Pg = s.prolongation()
    rng = np.random.default_rng(p + 10 * world)
    # --- layout, ownership, plans
    owned_all = np.concatenate([v.l2g[:v.n_true] for v in views])
    assert np.array_equal(np.sort(owned_all), np.arange(s.n_true))          # disjoint and covering
    eg = np.asarray(s.elem_dof_lex, dtype=np.int64)
    for v in views:
        assert v.n_true <= v.n_shared <= v.n_local == v.ndofs == v.l2g.size
        own, gh, con = v.l2g[:v.n_true], v.l2g[v.n_true:v.n_shared], v.l2g[v.n_shared:]
        assert np.all(np.diff(own) > 0) and np.all(np.diff(con) > 0) and np.all(own < s.n_true) and np.all(con >= s.n_true)
        assert np.all(gh < s.n_true) and np.all(v.owner[own] == v.rank) and np.all(v.owner[gh] != v.rank)
        key = v.owner[gh] * s.ndofs + gh
        assert np.all(np.diff(key) > 0)                                      # grouped by owner, then ascending
        in_elems = np.unique(eg[part == v.rank])
        assert np.isin(own, in_elems).all()                                  # an owner holds its dof through an element
        assert np.array_equal(con, in_elems[in_elems >= s.n_true])
        assert v.n_dep == int((~np.isin(gh, in_elems)).sum())
        assert np.array_equal(v.l2g[v.elem_dof_lex], eg[v.elems])
        assert v.C.shape == (v.n_local - v.n_shared, v.n_shared)
        assert v.mesh.ne == v.elems.size
        ess = v.l2g[v.ess_dofs()]
        assert np.array_equal(ess, np.intersect1d(np.asarray(s.ess_dofs(), dtype=np.int64), own))
        # send and recv lists match pairwise, in length and in global order
        assert v.nbr == sorted(v.nbr) and v.rank not in v.nbr
        recv_all = np.concatenate([r for r in v.recv]) if v.nbr else np.zeros(0, np.int64)
        assert np.array_equal(np.sort(recv_all), np.arange(v.n_true, v.n_shared))  # every ghost is received exactly once
        for k, q in enumerate(v.nbr):
            w = views[q]
            assert v.rank in w.nbr
            j = w.nbr.index(v.rank)
            assert np.array_equal(v.l2g[v.send[k]], w.l2g[w.recv[j]]) and np.array_equal(v.l2g[v.recv[k]], w.l2g[w.send[j]])
            assert np.all(v.send[k] < v.n_true) and np.all(np.diff(v.l2g[v.send[k]]) > 0) and np.all(np.diff(v.l2g[v.recv[k]]) > 0)
    # --- P: every rank's [I; C_loc] on its copies of the true dofs is the global P x at its dofs
    x = rng.uniform(-1, 1, s.n_true)
    ref = Pg @ x
    for v in views:
        lx = v.prolongation() @ x[v.l2g[:v.n_shared]]
        assert np.max(np.abs(lx - ref[v.l2g])) <= 1e-14 * max(1.0, np.max(np.abs(ref)))
    # --- P^T and |P|^T: fold locally, add the ghosts to their owners through the plan, compare on the owned dofs.  A sum has
    # at most a few dozen terms of size <= 1 from each of <= world ranks: 1e-13 of the largest entry is rounding with room.
    ly = [rng.uniform(-1, 1, v.n_local) for v in views]
    lg = np.zeros(s.ndofs)
    for v, l in zip(views, ly):
        np.add.at(lg, v.l2g, l)
    for absolute in (False, True):
        PT = (abs(Pg) if absolute else Pg).T
        want = PT @ lg
        t = [((abs(v.prolongation()) if absolute else v.prolongation()).T @ l) for v, l in zip(views, ly)]
        y = _halo_add(views, t)
        for v, yr in zip(views, y):
            assert np.max(np.abs(yr[:v.n_true] - want[v.l2g[:v.n_true]])) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("p", [1, 2, 3])
def test_dependency_only_ghosts_are_exercised(kind, p):
    """Mesh A, the eight children on rank 0 and the rest on rank 1: the masters of rank 0's constrained dofs lie on faces and
    edges of rank 1's elements, so rank 0 holds true dofs none of its elements contains -- except for H1 at order 1, whose only
    dofs are vertices: the corners of a master face or edge are corners of the children on it, so there every master is held
    through an element (counted on the CPU: 0).  An rcb cut of A has them for every kind and order."""
    _, _, hand = _view_set("A", kind, p, "hand")
    if kind == "h1" and p == 1:
        assert hand[0].n_dep == 0
    else:
        assert hand[0].n_dep > 0
    assert hand[1].n_dep == 0 and hand[1].n_local == hand[1].n_shared        # rank 1 has no constrained dofs at all
    _, _, cut = _view_set("A", kind, p, "rcb2")
    assert sum(v.n_dep for v in cut) > 0


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_rank_reproduces_the_space(name, kind):
    s = _space(name, kind, 2)
    v = PartitionedNCSpace(s, np.zeros(s.mesh.ne, dtype=np.int32), 0, 1)
    assert (v.n_true, v.n_shared, v.n_local) == (s.n_true, s.n_true, s.n_local) and v.n_dep == 0
    assert np.array_equal(v.l2g, np.arange(s.ndofs)) and np.array_equal(v.elem_dof_lex, s.elem_dof_lex)
    assert v.nbr == [] and v.send == [] and v.recv == []
    assert np.array_equal(v.C.indptr, s.C.indptr) and np.array_equal(v.C.indices, s.C.indices) and np.array_equal(v.C.data, s.C.data)
    assert np.array_equal(v.ess_dofs(), s.ess_dofs())
    if kind != "h1":
        assert np.array_equal(v.elem_sign_lex, s.elem_sign_lex)
    assert isinstance(v, KINDS[kind])
