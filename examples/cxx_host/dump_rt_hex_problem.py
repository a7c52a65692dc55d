"""Writes the arrays examples/cxx_host/rt_mass_hex.cpp reads: a hexahedral mesh with its elements handed over in seeded
rotations, the Raviart-Thomas space on it in its tensor description (lexicographic offsets + orientation flags), two
materials and the input vectors.
    python dump_rt_hex_problem.py problem.bin [p] [q1d]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.mesh import HexMesh, ogrid_cylinder  # noqa: E402

EPS = [np.array([[2.0, 0.3, 0.0], [0.3, 1.5, 0.1], [0.0, 0.1, 1.2]]), np.eye(3) * 3.1]
LAM = [1.9, 0.4]


def _rotation_perms():
    """The 24 proper rotations of the reference cube as permutations of the 27 lattice nodes i + 3 j + 9 k: the table of
    tests/util.py: hex_rotations() (same construction, same order; the examples do not import the test helpers -- keep the
    two in step)."""
    import itertools

    n = np.array([[i, j, k] for k in range(3) for j in range(3) for i in range(3)])
    perms = []
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
            perms.append(perm)
    return np.array(perms)


def problem(p=2, q1d=None):
    base = ogrid_cylinder(1, 3)
    ne = base.ne
    rot = np.random.default_rng(ne).permutation(np.arange(ne) % 24)
    nodes = np.take_along_axis(base.elem_nodes, _rotation_perms()[rot], axis=1)
    mesh = HexMesh(x=base.x, elem_nodes=nodes, attr=(1 + np.arange(ne) % 2).astype(np.int32), bdr_faces=base.bdr_faces,
                   bdr_attr=base.bdr_attr)
    mesh.check()
    sp = rthex.RTHexSpace(mesh, p)
    rng = np.random.default_rng(p)
    return dict(mesh=mesh, rt=sp, p=p, q1d=q1d or p + 1, eps=EPS, lam=LAM, x=rng.uniform(-1, 1, sp.ndofs),
                d0=rng.uniform(-1, 1, sp.ndofs))


def main(path, p=2, q1d=None):
    P = problem(p, q1d)
    mesh, sp = P["mesh"], P["rt"]
    arrays = [np.array([mesh.ne, mesh.x.shape[0], p, P["q1d"], sp.ndofs], dtype=np.int32),
              mesh.elem_nodes.astype(np.int32), mesh.x.astype(np.float64), mesh.attr.astype(np.int32),
              sp.elem_dof_lex.astype(np.int32), (sp.elem_sign_lex < 0).astype(np.uint8),
              np.concatenate([e.T.ravel() for e in P["eps"]]), np.asarray(P["lam"], np.float64), P["x"], P["d0"]]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[2:]]
    main(sys.argv[1], *a)
