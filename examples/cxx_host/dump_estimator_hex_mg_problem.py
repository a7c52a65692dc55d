"""Writes the arrays examples/cxx_host/estimate_hex_mg.cpp reads: the problem of dump_estimator_hex_complex_problem.py (rotated
hexahedral mesh, two materials each for the permittivity and the inverse permeability, complex fields E and B of order p) with
the Nedelec and the Raviart-Thomas space of EVERY order 1 .. p in their tensor descriptions: the p-multigrid hierarchies of the
flux projectors.  The mesh carries the rule of the finest level, q1d = p + 1.
    python dump_estimator_hex_mg_problem.py problem.bin [p]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dump_estimator_hex_complex_problem as cp  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402


def problem(p=2):
    P = cp.problem(p)
    P["nd_levels"] = [NDHexSpace(P["mesh"], l) for l in range(1, p)] + [P["nd"]]
    P["rt_levels"] = [rthex.RTHexSpace(P["mesh"], l) for l in range(1, p)] + [P["rt"]]
    return P


def main(path, p=2):
    P = problem(p)
    mesh = P["mesh"]
    sizes = [s.ndofs for s in P["nd_levels"]] + [s.ndofs for s in P["rt_levels"]]
    arrays = [np.array([mesh.ne, mesh.x.shape[0], p, P["q1d"]] + sizes, dtype=np.int32),
              mesh.elem_nodes.astype(np.int32), mesh.x.astype(np.float64), mesh.attr.astype(np.int32),
              np.concatenate([e.T.ravel() for e in P["eps"]]), np.concatenate([m.T.ravel() for m in P["muinv"]]),
              P["E"], P["E_im"], P["B"], P["B_im"]]
    for s in P["nd_levels"] + P["rt_levels"]:  # blobs 10 + 2 l (offsets), 11 + 2 l (flags): ND levels 1 .. p, then RT levels 1 .. p
        arrays += [s.elem_dof_lex.astype(np.int32), (s.elem_sign_lex < 0).astype(np.uint8)]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    main(sys.argv[1], *[int(v) for v in sys.argv[2:]])
