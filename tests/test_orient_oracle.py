"""Element orientation pinned through basis-invariant statements (CPU, the oracle alone).

Every parity test of the hexahedral kernels takes the dof maps, the signs and the face frames from palace_amd/fem/fespace.py
on both sides, on meshes whose elements all arrive in the orientation the mesh generator wrote.  Here every element is handed
over rotated (tests/util.py: rotate_elements -- the 24 proper rotations of the reference cube), which changes the element's own
frame and nothing else: vertices, edges and faces keep their numbers, so edge and face dofs (everything below int_base) keep
theirs and stand for the same functions, and only the interior dofs of an element change order and sign.  Hence, for x with
zero interior entries, the skeleton rows of K x, M x, (K + M) x are the same numbers on both meshes, the interior rows the
same up to order and sign inside each element, and the spectrum of K + M is the same.  A wrong sign, dof position or face
class (ou, ov, swap) in fespace.py breaks these.

Gates: 1e-12 (the project's oracle criterion, test/unit/test-libceed.cpp:245-282) on skeleton rows relative to max |y| and on
the spectrum relative to lambda_max; 1e-11 on |K G phi| / |M G phi| as tests/test_hiptmair_gpu.py.  The oracle alone measures
about 2e-15, 2e-15 and 1e-14."""
import numpy as np
import pytest

from oracle import palace_oracle as po
from palace_amd.fem.fespace import H1HexSpace, NDHexSpace, _face_orientation
from palace_amd.fem.mesh import HEX_FACES_UV, ogrid_cylinder
from tests import util

RTOL = 1e-12


def face_classes(mesh):
    """[6] sets of the (ou, ov, swap) classes met on every local face"""
    out = []
    for lf in range(6):
        ou, ov, sw = _face_orientation(mesh.verts[:, HEX_FACES_UV[lf]])
        out.append({(bool(a), bool(b), bool(c)) for a, b, c in zip(ou, ov, sw)})
    return out


def _with_attr(mesh):
    return type(mesh)(x=mesh.x, elem_nodes=mesh.elem_nodes, attr=(np.arange(mesh.ne) % 3 + 1).astype(np.int32),
                      bdr_faces=mesh.bdr_faces, bdr_attr=mesh.bdr_attr)


@pytest.fixture(scope="module")
def mesh10():
    return _with_attr(ogrid_cylinder(1, 2))


@pytest.fixture(scope="module")
def mesh80(cylinder_mesh):
    return _with_attr(cylinder_mesh)


@pytest.fixture(scope="module")
def mesh80_rot(mesh80):
    return util.rotate_elements(mesh80, util.seeded_rotations(mesh80.ne, 24))


def test_rotations_are_the_24_proper_ones():
    R, perm = util.hex_rotations()
    assert R.shape == (24, 3, 3) and perm.shape == (24, 27)
    for r, q in zip(R, perm):
        assert np.array_equal(np.abs(r).sum(axis=0), [1, 1, 1]) and np.array_equal(np.abs(r).sum(axis=1), [1, 1, 1])
        assert round(np.linalg.det(r)) == 1
        assert q[13] == 13 and np.array_equal(np.sort(q), np.arange(27))
    # closed under composition: a group of order 24
    keys = {tuple(q) for q in perm}
    assert len(keys) == 24 and all(tuple(a[b]) in keys for a in perm for b in perm)


def test_rotated_meshes_cover_every_face_class(mesh10, mesh80, mesh80_rot):
    ids = util.seeded_rotations(mesh80.ne, 24)
    assert set(ids) == set(range(24))
    every = {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    got = face_classes(mesh80_rot)
    print("classes per local face, as written:", [len(s) for s in face_classes(mesh80)], "rotated:", [len(s) for s in got])
    assert all(s == every for s in got)
    # the skeleton numbering does not move
    for p in (1, 3):
        a, b = NDHexSpace(mesh80, p), NDHexSpace(mesh80_rot, p)
        assert a.ndofs == b.ndofs and a.int_base == b.int_base
        for e in range(mesh80.ne):
            sa, sb = a.elem_dof_lex[e], b.elem_dof_lex[e]
            assert np.array_equal(np.sort(sa), np.sort(sb))
        h, g = H1HexSpace(mesh80, p), H1HexSpace(mesh80_rot, p)
        assert np.array_equal(np.sort(h.elem_dof_lex, axis=1), np.sort(g.elem_dof_lex, axis=1))
        assert np.array_equal(a.ess_dofs(), b.ess_dofs()) and np.array_equal(h.ess_dofs(), g.ess_dofs())
    # one uniform rotation for all elements, every one of the 24
    seen = [set() for _ in range(6)]
    for r in range(24):
        m = util.rotate_elements(mesh10, r)
        for lf, s in enumerate(face_classes(m)):
            seen[lf] |= s
    assert all(s == every for s in seen)


def _forms(nattr):
    _, b_a = util.make_ctx("aniso", nattr=nattr)
    _, b_n = util.make_ctx("scalar", nattr=nattr)
    return (("hdiv", b_a), ("hcurl", b_a), ("hdivmass", np.concatenate([b_n, b_a])), ("hdivmass", np.concatenate([b_a, b_a])))


def _skeleton_check(mesh, rot, p, worst):
    q1d = p + 1
    a, b = NDHexSpace(mesh, p), NDHexSpace(rot, p)
    ga, gb = util.oracle_geom(mesh, q1d), util.oracle_geom(rot, q1d)
    x = np.random.default_rng(10 + p).uniform(-1, 1, a.ndofs)
    x[a.int_base:] = 0.0
    for qf, blob in _forms(3):
        ya = util.oracle_apply_c(a, ga, qf, blob, x, q1d)
        yb = util.oracle_apply_c(b, gb, qf, blob, x, q1d)
        scale = np.abs(ya).max()
        err = np.abs(ya[:a.int_base] - yb[:a.int_base]).max() / scale
        ia = np.sort(np.abs(ya[a.int_base:]).reshape(mesh.ne, -1), axis=1)
        ib = np.sort(np.abs(yb[a.int_base:]).reshape(mesh.ne, -1), axis=1)
        erri = np.abs(ia - ib).max() / scale if ia.size else 0.0
        worst[0], worst[1] = max(worst[0], err), max(worst[1], erri)
        assert err < RTOL and erri < RTOL, (p, qf, err, erri)
        if p > 1:
            assert not np.array_equal(ya[a.int_base:], yb[a.int_base:])  # (the interior frame did change)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_skeleton_rows_uniform_rotations(mesh10, p):
    """One rotation for all ten elements, each of the 24: K, M and K + M with a tensor coefficient."""
    worst = [0.0, 0.0]
    for r in range(1, 24):
        _skeleton_check(mesh10, util.rotate_elements(mesh10, r), p, worst)
    print(f"p = {p}: skeleton rows {worst[0]:.2e}, interior |y| per element {worst[1]:.2e} (relative to max |y|)")


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_skeleton_rows_rotation_per_element(mesh80, mesh80_rot, p):
    worst = [0.0, 0.0]
    _skeleton_check(mesh80, mesh80_rot, p, worst)
    print(f"p = {p}: skeleton rows {worst[0]:.2e}, interior |y| per element {worst[1]:.2e} (relative to max |y|)")


def test_spectrum_is_unchanged(mesh10):
    p, q1d = 2, 3
    rot = util.rotate_elements(mesh10, util.seeded_rotations(mesh10.ne, 3))
    _, b_a = util.make_ctx("aniso", nattr=3)
    blob = np.concatenate([b_a, b_a])
    lam = []
    for m in (mesh10, rot):
        nd = NDHexSpace(m, p)
        assert nd.ndofs == 320
        g = util.oracle_geom(m, q1d)
        A = np.stack([util.oracle_apply_c(nd, g, "hdivmass", blob, e, q1d) for e in np.eye(nd.ndofs)], axis=1)
        assert np.abs(A - A.T).max() < 1e-13 * np.abs(A).max()
        lam.append(np.linalg.eigvalsh(0.5 * (A + A.T)))
    assert lam[0][0] > 0.0
    err = np.abs(lam[0] - lam[1]).max() / lam[0][-1]
    print(f"spectrum of K + M, 320 dofs: {err:.2e} of lambda_max = {lam[0][-1]:.4g}")
    assert err < RTOL


def _interp(c, f):
    return po.InterpOracle(c.elem_dof_lex, c.elem_sign_lex, f.elem_dof_lex, f.elem_sign_lex, c.ndofs, f.ndofs, po.nd_hex_interp_lex(c.p, f.p))


def _gradient(h1, nd):
    ones = np.ones(h1.elem_dof_lex.shape, dtype=np.int8)
    return po.InterpOracle(h1.elem_dof_lex, ones, nd.elem_dof_lex, nd.elem_sign_lex, h1.ndofs, nd.ndofs, po.nd_hex_gradient_lex(nd.p))


@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (3, 4)])
def test_p_transfer_skeleton_rows(mesh80, mesh80_rot, pc, pf):
    rng = np.random.default_rng(pc + pf)
    ca, fa, cb, fb = NDHexSpace(mesh80, pc), NDHexSpace(mesh80, pf), NDHexSpace(mesh80_rot, pc), NDHexSpace(mesh80_rot, pf)
    Pa, Pb = _interp(ca, fa), _interp(cb, fb)
    xa, xb = rng.uniform(-1, 1, ca.ndofs), rng.uniform(-1, 1, ca.ndofs)
    xb[:ca.int_base] = xa[:ca.int_base]  # any interior entries: they have no tangential trace on the skeleton
    ya, yb = Pa.mult(xa), Pb.mult(xb)
    err = np.abs(ya[:fa.int_base] - yb[:fa.int_base]).max() / np.abs(ya).max()
    xf = rng.uniform(-1, 1, fa.ndofs)
    xf[fa.int_base:] = 0.0
    za, zb = Pa.mult_transpose(xf), Pb.mult_transpose(xf)
    errt = np.abs(za[:ca.int_base] - zb[:ca.int_base]).max() / np.abs(za).max()
    print(f"P {pc} -> {pf}: skeleton rows {err:.2e}, of the transpose {errt:.2e}")
    assert err < RTOL and errt < RTOL


@pytest.mark.parametrize("p", [1, 2, 3])
def test_gradient_skeleton_rows_and_curl_of_gradient(mesh80, mesh80_rot, p):
    q1d = p + 1
    rng = np.random.default_rng(20 + p)
    ha, na, hb, nb = H1HexSpace(mesh80, p), NDHexSpace(mesh80, p), H1HexSpace(mesh80_rot, p), NDHexSpace(mesh80_rot, p)
    assert ha.int_base == hb.int_base
    Ga, Gb = _gradient(ha, na), _gradient(hb, nb)
    phi = rng.uniform(-1, 1, ha.ndofs)
    phi[ha.int_base:] = 0.0
    ga, gb = Ga.mult(phi), Gb.mult(phi)
    err = np.abs(ga[:na.int_base] - gb[:na.int_base]).max() / np.abs(ga).max()
    # curl grad = 0 on the rotated mesh, any phi
    phi = rng.uniform(-1, 1, hb.ndofs)
    g = Gb.mult(phi)
    geom = util.oracle_geom(mesh80_rot, q1d)
    _, b_i = util.make_ctx("identity")
    _, b_s = util.make_ctx("scalar", nattr=3)
    kg = util.oracle_apply_c(nb, geom, "hdiv", b_i, g, q1d)
    mg = util.oracle_apply_c(nb, geom, "hcurl", b_s, g, q1d)
    ratio = np.abs(kg).max() / np.abs(mg).max()
    print(f"G p = {p}: skeleton rows {err:.2e}, |K G phi| / |M G phi| = {ratio:.2e}")
    assert err < RTOL
    assert ratio < 1e-11


# (space, p, capacity of the streaming index of the kernel that order takes: pa_stream_host.hpp kIdxMaxRuns = 20 for the four-point
# H(curl) kernel, kWideMaxRuns = 24 for the five-point one, kIdxWords - kIdxStart0H1 = 28 for the H1 kernel)
CAPACITY_CASES = [("nd", 2, 20), ("nd", 3, 20), ("nd", 4, 24), ("h1", 3, 28)]


@pytest.mark.parametrize("kind,p,cap", CAPACITY_CASES)
def test_fragmented_numberings_reach_the_index_capacity(cylinder_mesh, kind, p, cap):
    """The inputs of the capacity tests of tests/test_orient_gpu.py: rotating elements cannot reach the capacity (an element's
    dofs stay grouped by mesh entity: at most 18 runs in ND, 24 in H1 on this mesh), exchanging single dofs between far blocks
    does -- exactly at the capacity, and two runs above it."""
    space = (NDHexSpace if kind == "nd" else H1HexSpace)(cylinder_mesh, p)
    base = util.element_runs(space.elem_dof_lex).max()
    assert base == (18 if kind == "nd" else 24)
    rot = (NDHexSpace if kind == "nd" else H1HexSpace)(util.rotate_elements(cylinder_mesh, util.seeded_rotations(80, 24)), p)
    assert util.element_runs(rot.elem_dof_lex).max() <= base
    for where, target in (("interior", cap), ("interior", cap + 2), ("faces", cap)):
        perm, runs = util.fragmenting_permutation(space, where, target)
        print(kind, p, where, "runs", base, "->", runs.max(), "dofs moved", int((perm != np.arange(space.ndofs)).sum()))
        assert runs.max() == target
        assert np.array_equal(runs, util.element_runs(util.renumbered(space, perm).elem_dof_lex))
    full = np.random.default_rng(5).permutation(space.ndofs)
    assert util.element_runs(util.renumbered(space, full).elem_dof_lex).min() > cap
