"""The inputs the GPU tests of the sum-factorised RT hexahedra rest on (tests/test_rt_hex_gpu.py): RTHexSpace and the oracle on
the two meshes with every element handed over in a seeded rotation.  CPU only."""
import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import util


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("p", [1, 2, 3])
def test_rt_hex_rotated_energy_identity_and_face_agreement(kind, p):
    """tests/test_rt_space.py::test_rt_hex_discrete_curl_energy_identity on the rotated meshes: the flux dofs computed by the
    elements sharing a face agree, (K u, u) = (M_RT C u, C u), div curl = 0; both face signs occur and the Jacobi diagonal is
    positive."""
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace

    mesh, q1d = ru.mesh(kind), p + 1
    nd, rt_ = NDHexSpace(mesh, p), ru.space(kind, p)
    ogeom = ru.ogeom(kind, q1d)
    one = po.CoeffCtx()
    interp, curl = po.nd_hex_dense_tables(p, q1d, np.arange(nd.P))
    K = po.CeedOperatorOracle(nd.ndofs, nd.elem_dof_lex, nd.elem_sign_lex < 0, interp, curl, ogeom, po.QF_HDIV, one)
    rint, rdiv = ru.tables(p, q1d)
    M = po.CeedOperatorOracle(rt_.ndofs, rt_.elem_dof_lex, rt_.elem_sign_lex < 0, rint, rint, ogeom, po.QF_HDIV, one)
    Cm = rthex.hex_curl_matrix(p)
    dom = dict(offsets=nd.elem_dof_lex, lsize=nd.ndofs, orients=nd.elem_sign_lex < 0)
    C = po.DenseInterpOracle(dom, rt_.restriction(interp_range=True), Cm)
    u = np.random.default_rng(11).uniform(-1, 1, nd.ndofs)
    b = C.mult(u)
    ue = (u[nd.elem_dof_lex] * nd.elem_sign_lex) @ Cm.T
    ge = b[rt_.elem_dof_lex] * rt_.elem_sign_lex
    assert np.abs(ue - ge).max() < 1e-10 * np.abs(ue).max()
    e_k = u @ K.apply_add(u, np.zeros(nd.ndofs))
    e_m = b @ M.apply_add(b, np.zeros(rt_.ndofs))
    assert abs(e_k - e_m) < 1e-11 * abs(e_k)
    assert np.abs(ue @ rdiv.T).max() < 1e-9 * np.abs(ue).max()
    cnt = np.bincount(rt_.elem_dof_lex.ravel(), minlength=rt_.ndofs)
    assert cnt.min() == 1 and cnt.max() == 2
    neg = (rt_.elem_sign_lex < 0).mean()
    assert 0.1 < neg < 0.6  # both face signs occur
    assert set(np.unique(mesh.attr)) == {1, 2}
    assert ru.oracle_diag(kind, p, q1d, "mass").min() > 0.0


def test_rotated_meshes_cover_partial_waves():
    """80 elements are whole blocks at four and five points per direction, 15 leave a partial wave at every rule."""
    assert ru.mesh("cyl80").ne == 80 and ru.mesh("ogrid15").ne == 15
    rot = util.seeded_rotations(80, 80)
    assert len(set(rot.tolist())) == 24
