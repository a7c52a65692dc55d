"""Shared inputs of the Raviart-Thomas hexahedron tests (test_rt_hex_gpu.py, test_rt_hex_rotated.py, test_cxx_rt_hex_gpu.py):
the two rotated meshes, the spaces, dense tables and oracle operators on them, each built once per session."""
import os

import numpy as np

from oracle import palace_oracle as po
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ("cyl80", "ogrid15")
_cache = {}


def mesh(kind):
    """cyl80: the 80-element cylinder fixture (whole blocks at four and five points per direction); ogrid15: ogrid_cylinder(1, 3),
    15 elements (a partial wave and block at every rule).  Two attributes in turn, every element handed over in a seeded rotation."""
    if ("mesh", kind) not in _cache:
        from palace_amd.fem.mesh import HexMesh, ogrid_cylinder

        if kind == "cyl80":
            d = np.load(os.path.join(ROOT, "tests", "golden", "cylinder_hex_mesh.npz"))
            x, nodes, bf, ba, seed = d["x"], d["elem_nodes"].astype(np.int64), d["bdr_faces"], d["bdr_attr"], 80
        else:
            m = ogrid_cylinder(1, 3)
            x, nodes, bf, ba, seed = m.x, m.elem_nodes, m.bdr_faces, m.bdr_attr, 15
        ne = nodes.shape[0]
        fresh = HexMesh(x=x, elem_nodes=nodes, attr=(1 + np.arange(ne) % 2).astype(np.int32), bdr_faces=bf, bdr_attr=ba)
        fresh.check()
        _cache["mesh", kind] = util.rotate_elements(fresh, util.seeded_rotations(ne, seed))
    return _cache["mesh", kind]


def space(kind, p):
    if ("space", kind, p) not in _cache:
        from palace_amd.fem import rthex

        _cache["space", kind, p] = rthex.RTHexSpace(mesh(kind), p)
    return _cache["space", kind, p]


def tables(p, q1d):
    """(values [3, Q, P], divergence [Q, P]) in tensor order."""
    if ("tab", p, q1d) not in _cache:
        from palace_amd.fem import rthex
        from palace_amd.fem.basis1d import gauss_legendre

        _cache["tab", p, q1d] = rthex.rt_hex_tables(p, gauss_legendre(q1d)[0])
    return _cache["tab", p, q1d]


def ogeom(kind, q1d):
    if ("ogeom", kind, q1d) not in _cache:
        _cache["ogeom", kind, q1d] = util.oracle_geom(mesh(kind), q1d)
    return _cache["ogeom", kind, q1d]


def div_ctx():
    """Two-material scalar context of the divergence term."""
    return po.CoeffCtx(attr_mat=[1, 0], mat_coeff=[np.array([1.9]), np.array([0.4])], dim=1)


def mass_ctx(mass):
    """util.make_ctx(mass, 2); "nonsym_t": the non-symmetric context with every material matrix transposed."""
    if mass != "nonsym_t":
        return util.make_ctx(mass, 2)[0]
    rng = np.random.default_rng(9)  # (the matrix of util.make_ctx("nonsym"))
    A = rng.uniform(-1, 1, (3, 3)) + 3.0 * np.eye(3)
    return po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[A.T.copy(), np.array([0.7])], a=1.1)


def oracle(kind, p, q1d, form, mass="aniso"):
    """CeedOperatorOracle of `form` in ("mass", "divdiv", "divdivmass") on the RT space."""
    key = ("orc", kind, p, q1d, form, mass)
    if key not in _cache:
        sp = space(kind, p)
        rint, rdiv = tables(p, q1d)
        _, wts = po.hex_quadrature(q1d)
        cm = mass_ctx(mass)
        args = (sp.ndofs, sp.elem_dof_lex, sp.elem_sign_lex < 0)
        g = ogeom(kind, q1d)
        if form == "mass":
            o = po.CeedOperatorOracle(*args, rint, rint, g, po.QF_HDIV, cm)
        elif form == "divdiv":
            o = po.CeedOperatorOracle(*args, rint, rdiv, g, po.QF_L2_1, div_ctx(), qw=wts, deriv_comps=1)
        else:
            o = po.CeedOperatorOracle(*args, rint, rdiv, g, po.QF_L2MASS, cm, div_ctx(), qw=wts, deriv_comps=1)
        _cache[key] = o
    return _cache[key]


def vector(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def oracle_mult(kind, p, q1d, form, mass="aniso", x=None):
    """(x, A x) with the fixed input of the parity tests (cached), or with the given x."""
    o = oracle(kind, p, q1d, form, mass)
    if x is not None:
        return x, o.apply_add(x, np.zeros(o.lsize))
    key = ("mult", kind, p, q1d, form, mass)
    if key not in _cache:
        x = vector(o.lsize, 100 * p + q1d)
        _cache[key] = (x, o.apply_add(x, np.zeros(o.lsize)))
    return _cache[key]


def oracle_diag(kind, p, q1d, form, mass="aniso"):
    key = ("diag", kind, p, q1d, form, mass)
    if key not in _cache:
        _cache[key] = oracle(kind, p, q1d, form, mass).diagonal()
    return _cache[key]


def boundary_dofs(kind, p):
    """The dofs of the boundary faces."""
    sp = space(kind, p)
    faces = np.nonzero(sp.mesh.boundary_face_mask)[0]
    return (sp.face_base + faces[:, None] * p * p + np.arange(p * p)[None, :]).ravel().astype(np.int32)
