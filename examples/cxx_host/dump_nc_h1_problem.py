"""The H1 side of the problem of dump_nc_problem.py (same refined cylinder, same orders) for solve_nc_assembled.cpp, which needs
it for LinearSolver::BOOMER_AMG on an H1 problem and as the auxiliary hierarchy of LinearSolver::AMS: for every level p = 1 ..
order the H1 space in the layout of a space with hanging-node constraints -- true dofs first -- with its element -> dof table
(tensor order), its essential true dofs and the constraint matrix C of P = [I; C] in CSR.  The vertex coordinates follow from
the mesh of the first blob and the order-1 table (Mesh::VertexCoordinates).
Usage: python dump_nc_h1_problem.py out.bin [order]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from dump_nc_problem import problem as nd_problem  # noqa: E402
from palace_amd.fem import nchex  # noqa: E402
from palace_amd.fem.fespace import H1HexSpace  # noqa: E402


def problem(order=2):
    """(refined mesh, [constrained H1 space of order 1 .. order]) on the mesh of dump_nc_problem.problem."""
    mesh, _ = nd_problem(1)
    return mesh, [nchex.NCSpace(H1HexSpace(mesh, q)) for q in range(1, order + 1)]


def main(path, p=2):
    mesh, spaces = problem(p)
    arrays = [np.array([p, len(spaces)] + [s.p for s in spaces], dtype=np.int32)]
    for h1 in spaces:
        C = h1.C.tocsr()
        arrays += [np.array([h1.n_local, h1.n_true], dtype=np.int32), h1.elem_dof_lex.astype(np.int32), h1.ess_dofs().astype(np.int32),
                   C.indptr.astype(np.int32), C.indices.astype(np.int32), C.data.astype(np.float64)]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    main(sys.argv[1], *[int(v) for v in sys.argv[2:]])
