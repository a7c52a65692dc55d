"""Write what Palace's MFEM side would hand over after ONE nonconformal refinement step of the reference cylinder
(tests/golden/cylinder_hex_mesh.npz, 80 curved hex27 elements; a seeded quarter of them refined: hanging faces and edges)
into one binary file for the C++ host example solve_nc.cpp: the leaf elements of the refined mesh and, for every multigrid
level p = 1 .. order, the Nedelec space in the layout of a space with hanging-node constraints -- true dofs first, then the
constrained ones -- with its element -> dof table, orientation flags, tensor -> native dof map, essential (PEC) true dofs and
the constraint matrix C of the conforming prolongation P = [I; C] in CSR (palace_amd/fem/nchex.py: what
mfem::FiniteElementSpace::GetConformingProlongation() is there).
Usage: python dump_nc_problem.py out.bin [order]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from palace_amd.fem import nchex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import HexMesh  # noqa: E402


def problem(order=2):
    """(refined mesh, [constrained Nedelec space of order 1 .. order])."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "cylinder_hex_mesh.npz"))
    m0 = HexMesh(x=z["x"], elem_nodes=z["elem_nodes"].astype(np.int64), attr=z["attr"].astype(np.int32))
    marked = np.sort(np.random.default_rng(11).permutation(m0.ne)[: m0.ne // 4])
    mesh = nchex.refine_local(m0, marked)
    return mesh, [nchex.NCSpace(NDHexSpace(mesh, q)) for q in range(1, order + 1)]


def main(path, p=2):
    mesh, spaces = problem(p)
    orders = [s.p for s in spaces]
    arrays = [np.array([mesh.ne, mesh.x.shape[0], p, len(orders)] + orders, dtype=np.int32),
              mesh.elem_nodes.astype(np.int32), mesh.x.astype(np.float64), mesh.attr.astype(np.int32)]
    for nd in spaces:
        off, ori = nd.native_restriction()
        C = nd.C.tocsr()
        arrays += [np.array([nd.n_local, nd.n_true], dtype=np.int32), off.astype(np.int32), ori.astype(np.uint8),
                   np.asarray(nd.dof_map_native(), dtype=np.int32), nd.ess_dofs().astype(np.int32),
                   C.indptr.astype(np.int32), C.indices.astype(np.int32), C.data.astype(np.float64)]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    main(sys.argv[1], *[int(v) for v in sys.argv[2:]])
