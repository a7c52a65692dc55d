"""Writes the arrays examples/cxx_host/estimate_hex_complex.cpp reads: the problem of dump_estimator_hex_problem.py (rotated
hexahedral mesh, Nedelec and Raviart-Thomas space of order p in their tensor descriptions, two materials each for the
permittivity and the inverse permeability) with complex fields E (H(curl)) and B (H(div)), real and imaginary parts.
    python dump_estimator_hex_complex_problem.py problem.bin [p]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dump_estimator_hex_problem as ep  # noqa: E402


def problem(p=2):
    P = ep.problem(p)
    rng = np.random.default_rng(20 + p)
    P["E_im"] = rng.uniform(-1, 1, P["nd"].ndofs)
    P["B_im"] = rng.uniform(-1, 1, P["rt"].ndofs)
    return P


def main(path, p=2):
    P = problem(p)
    mesh, nd, sp = P["mesh"], P["nd"], P["rt"]
    arrays = [np.array([mesh.ne, mesh.x.shape[0], p, P["q1d"], nd.ndofs, sp.ndofs], dtype=np.int32),
              mesh.elem_nodes.astype(np.int32), mesh.x.astype(np.float64), mesh.attr.astype(np.int32),
              nd.elem_dof_lex.astype(np.int32), (nd.elem_sign_lex < 0).astype(np.uint8),
              sp.elem_dof_lex.astype(np.int32), (sp.elem_sign_lex < 0).astype(np.uint8),
              np.concatenate([e.T.ravel() for e in P["eps"]]), np.concatenate([m.T.ravel() for m in P["muinv"]]),
              P["E"], P["E_im"], P["B"], P["B_im"]]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    main(sys.argv[1], *[int(v) for v in sys.argv[2:]])
