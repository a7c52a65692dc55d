"""Raviart-Thomas spaces with hanging-face constraints (fem/nchex.py: NCSpace of an RTHexSpace) on the three meshes of
tests/nc_util.py at orders 1 to 3, on the host: the counts, the shape of the rows, the nodal interpolant of a field the space
contains, the commuting identity with the Nedelec constraints through the local discrete curl, and the divergence of a curl."""
import numpy as np
import pytest

from palace_amd.fem import nchex, rthex
from tests import nc_util as nu
from tests import rt_nc_util as rn

CASES = [(m, p) for m in "ABC" for p in (1, 2, 3)]
MASTER_FACES = {"A": 3, "B": 13, "C": 76}
CONSTRAINED = {"A": (12, 48, 108), "B": (52, 208, 468), "C": (304, 1216, 2736)}


@pytest.mark.parametrize("name,p", CASES)
def test_counts_and_rows(name, p):
    """4 p^2 constrained dofs per master face, p^2 entries per row, every column a true dof; +-1/4 at order 1."""
    rt = rn.rt_space(name, p)
    assert isinstance(rt, nchex.NCRTHexSpace)
    mesh = nu.nc_mesh(name)
    assert mesh.master_faces.size == MASTER_FACES[name]
    n_con = rt.n_local - rt.n_true
    assert n_con == CONSTRAINED[name][p - 1] == 4 * p * p * MASTER_FACES[name]
    assert rt.n_local == rt.broken.ndofs and rt.C.shape == (n_con, rt.n_true)
    assert np.all(np.diff(rt.C.indptr) == p * p)
    assert rt.C.indices.min() >= 0 and rt.C.indices.max() < rt.n_true          # no chains
    assert np.array_equal(np.sort(rt.broken_perm), np.arange(rt.n_local))
    assert np.array_equal(rt.elem_dof_lex, rt.broken_perm[rt.broken.elem_dof_lex])
    # only slave-face dofs are constrained
    slave = (rt.broken.face_base + mesh.slave_faces[:, None] * p * p + np.arange(p * p)[None, :]).ravel()
    assert np.array_equal(np.sort(rt.broken_perm[slave]), rt.n_true + np.arange(n_con))
    assert rt.ess_dofs().size == 0
    if p == 1:
        assert np.array_equal(np.abs(rt.C.data), np.full(n_con, 0.25))
    P = rt.prolongation()
    assert P.shape == (rt.n_local, rt.n_true)
    head = P[: rt.n_true].tocoo()
    assert head.nnz == rt.n_true and np.array_equal(head.row, head.col) and np.all(head.data == 1.0)


def test_conforming_mesh_has_no_constraints():
    rt = nchex.NCSpace(rthex.RTHexSpace(nchex.refine_local(nu.start_mesh("A"), []), 2))
    assert rt.C.shape == (0, rt.n_true) and rt.n_true == rt.n_local == rt.broken.ndofs
    rt = nchex.NCSpace(rthex.RTHexSpace(nu.start_mesh("C"), 1))
    assert rt.C.shape[0] == 0


@pytest.mark.parametrize("name,p", CASES)
def test_interpolant_of_a_contained_field(name, p):
    """u = P R u for the nodal interpolant (the contravariant Piola pull-back at the dof nodes) of a field whose normal flux
    density on every face lies in the trace space.  On the affine blocks any constant field does.  On the cylinder the
    elements are curved in the plane and extruded along z, so a constant in-plane field has the flux density 0 on the
    horizontal faces and h (y_t, -x_t) . u on the vertical ones with t the in-plane tangent: the refined faces are ruled along
    z and straight along t, so this is constant on them, in the trace space of every order."""
    rt = rn.rt_space(name, p)
    c = np.array([0.3, -1.1, 0.0 if name == "C" else 0.7])
    u = rn.rt_interpolate(rt, lambda x: np.tile(c, (x.shape[0], 1)))
    assert np.abs(u[rt.n_true:]).max() > 0.01 * np.abs(u).max()
    err = np.abs(rt.prolongation() @ u[: rt.n_true] - u).max() / np.abs(u).max()
    print(f"{name} p={p}: |P R u - u| / |u| = {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("name,p", CASES)
def test_curl_commutes_with_the_constraints(name, p):
    """P_rt R_rt C_loc P_nd x = C_loc P_nd x: the curl of a conforming Nedelec field has the constrained flux dofs its master
    traces give.  1e-12 relative to the largest entry (measured 1.4e-16 to 5e-16)."""
    Ct, nd, rt = rn.true_curl(name, p)
    x = np.random.default_rng(10 * p + ord(name)).uniform(-1, 1, nd.n_true)
    local = rn.local_curl(nd, rt) @ (nd.prolongation() @ x)
    got = rt.prolongation() @ (Ct @ x)
    err = np.abs(got - local).max() / np.abs(local).max()
    print(f"{name} p={p}: {err:.2e}")
    assert np.abs(local[rt.n_true:]).max() > 0.0
    assert err < 1e-12


@pytest.mark.parametrize("name,p", CASES)
def test_divergence_of_the_curl_vanishes(name, p):
    """div (P_rt R_rt C_loc P_nd x) = 0 element by element (the reference divergence at the Gauss points; the physical one is
    that over det J), to 1e-11 of the largest flux dof."""
    from palace_amd.fem.basis1d import gauss_legendre

    Ct, nd, rt = rn.true_curl(name, p)
    x = np.random.default_rng(20 * p + ord(name)).uniform(-1, 1, nd.n_true)
    u = rt.prolongation() @ (Ct @ x)
    _, div = rthex.rt_hex_tables(p, gauss_legendre(p + 1)[0])
    d = np.einsum("qp,ep->eq", div, u[rt.elem_dof_lex] * rt.elem_sign_lex)
    err = np.abs(d).max() / np.abs(u).max()
    print(f"{name} p={p}: max |div| / max |u| = {err:.2e}")
    assert err < 1e-11


def test_new_symbols_are_exported():
    import __graft_entry__ as ge

    ge.build()
    from palace_amd import lib

    L = lib.load()
    for name in ("pa_conform_prolongate2", "pa_conform_restrict2", "pa_curl_create_conforming"):
        assert hasattr(L, name), name
