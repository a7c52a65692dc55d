"""One file per rank for examples/cxx_host/solve_nc_ranks.cpp: the problem of dump_nc_problem.py (the reference cylinder with a
seeded quarter of its elements refined once, hanging faces and edges) cut into `world` parts by recursive coordinate bisection.
A rank's file holds its elements and, for every multigrid level p = 1 .. order, its view of the constrained Nedelec space
(palace_amd/fem/ncpart.py): the local vector is owned true dofs, ghost true dofs grouped by owner, constrained dofs; the
element -> dof table, orientation flags, tensor -> native dof map, essential (PEC) true dofs among the owned ones, the local
constraint matrix C [n_local - n_shared, n_shared] in CSR and the halo plan over the prefix [0, n_shared) -- what Palace's
ParMesh / ParFiniteElementSpace hold on a rank after a nonconformal refinement.
Usage: python dump_nc_problem_ranks.py prefix world [order]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from dump_nc_problem import problem  # noqa: E402
from dump_problem_ranks import plan_arrays  # noqa: E402
from palace_amd.fem import rcb  # noqa: E402
from palace_amd.fem.ncpart import PartitionedNCSpace  # noqa: E402


def views(world, p=2):
    """(refined mesh, global constrained spaces of order 1 .. p, [rank][level] views)."""
    mesh, spaces = problem(p)
    part = rcb.rcb(mesh.elem_coords().mean(axis=1), world)
    return mesh, spaces, [[PartitionedNCSpace(s, part, r, world) for s in spaces] for r in range(world)]


def main(prefix, world, p=2):
    mesh, spaces, per_rank = views(world, p)
    orders = [s.p for s in spaces]
    for rank, vs in enumerate(per_rank):
        sub = vs[0].mesh
        # the rank's elements on the nodes of the whole mesh (unused nodes are harmless: the geometry is per element)
        arrays = [np.array([sub.ne, sub.x.shape[0], p, len(orders)] + orders, dtype=np.int32),
                  sub.elem_nodes.astype(np.int32), sub.x.astype(np.float64), sub.attr.astype(np.int32)]
        for v in vs:
            off, ori = v.native_restriction()
            C = v.C.tocsr()
            arrays += [np.array([v.n_local, v.n_true, v.n_shared], dtype=np.int32), off.astype(np.int32), ori.astype(np.uint8),
                       np.asarray(v.dof_map_native(), dtype=np.int32), v.ess_dofs().astype(np.int32),
                       C.indptr.astype(np.int32), C.indices.astype(np.int32), C.data.astype(np.float64)]
            arrays += plan_arrays(v)
        with open(f"{prefix}.{rank}", "wb") as f:
            f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
            for a in arrays:
                a = np.ascontiguousarray(a)
                f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
                f.write(a.tobytes())


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), *[int(v) for v in sys.argv[3:]])
