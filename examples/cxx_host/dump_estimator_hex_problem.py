"""Writes the arrays examples/cxx_host/estimate_hex.cpp reads: the rotated hexahedral mesh of dump_rt_hex_problem.py, the
Nedelec and the Raviart-Thomas space of order p on it in their tensor descriptions (lexicographic offsets + orientation flags),
two materials each for the permittivity and the inverse permeability, and the fields E (H(curl)) and B (H(div)).
    python dump_estimator_hex_problem.py problem.bin [p]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dump_rt_hex_problem as rp  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402

EPS = rp.EPS
MUINV = [np.array([[0.9, -0.1, 0.05], [-0.1, 1.3, 0.0], [0.05, 0.0, 0.7]]), np.eye(3) * 0.8]


def problem(p=2):
    P = rp.problem(p)
    nd = NDHexSpace(P["mesh"], p)
    rng = np.random.default_rng(10 + p)
    return dict(mesh=P["mesh"], nd=nd, rt=P["rt"], p=p, q1d=p + 1, eps=EPS, muinv=MUINV, E=rng.uniform(-1, 1, nd.ndofs),
                B=rng.uniform(-1, 1, P["rt"].ndofs))


def main(path, p=2):
    P = problem(p)
    mesh, nd, sp = P["mesh"], P["nd"], P["rt"]
    arrays = [np.array([mesh.ne, mesh.x.shape[0], p, P["q1d"], nd.ndofs, sp.ndofs], dtype=np.int32),
              mesh.elem_nodes.astype(np.int32), mesh.x.astype(np.float64), mesh.attr.astype(np.int32),
              nd.elem_dof_lex.astype(np.int32), (nd.elem_sign_lex < 0).astype(np.uint8),
              sp.elem_dof_lex.astype(np.int32), (sp.elem_sign_lex < 0).astype(np.uint8),
              np.concatenate([e.T.ravel() for e in P["eps"]]), np.concatenate([m.T.ravel() for m in P["muinv"]]), P["E"], P["B"]]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    main(sys.argv[1], *[int(v) for v in sys.argv[2:]])
