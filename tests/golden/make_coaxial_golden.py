"""Generate tests/golden/coaxial_matched.npz: the reference's coaxial transient example as arrays -- the mesh
(examples/coaxial/mesh/coaxial.msh: 256 hex27, 544 boundary quadrilaterals with attributes 2 = PEC, 3 and 4 = the two ports) as
palace_amd.fem.mesh.read_gmsh22 returns it, and the columns of the regression outputs of coaxial_matched.json
(test/data/regression/ref/coaxial/matched/{port-V,port-I,domain-E}.csv, 201 rows).  Needs a checkout of the reference (as
tests/golden/make_golden.py does); no test reads it:  python tests/golden/make_coaxial_golden.py <reference root>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(ref):
    from palace_amd.fem.mesh import read_gmsh22

    m = read_gmsh22(os.path.join(ref, "examples", "coaxial", "mesh", "coaxial.msh"))
    out = dict(x=m.x, elem_nodes=m.elem_nodes.astype(np.int32), attr=m.attr.astype(np.int32),
               bdr_faces=m.bdr_faces.astype(np.int32), bdr_attr=m.bdr_attr.astype(np.int32))
    d = os.path.join(ref, "test", "data", "regression", "ref", "coaxial", "matched")
    V = np.loadtxt(os.path.join(d, "port-V.csv"), delimiter=",", skiprows=1)
    I = np.loadtxt(os.path.join(d, "port-I.csv"), delimiter=",", skiprows=1)
    E = np.loadtxt(os.path.join(d, "domain-E.csv"), delimiter=",", skiprows=1)
    assert V.shape == (201, 4) and I.shape == (201, 4) and E.shape[0] == 201
    assert np.array_equal(V[:, 0], I[:, 0]) and np.array_equal(V[:, 0], E[:, 0])
    out.update(t_ns=V[:, 0], V_inc1=V[:, 1], V1=V[:, 2], V2=V[:, 3], I_inc1=I[:, 1], I1=I[:, 2], I2=I[:, 3], E_elec=E[:, 1], E_mag=E[:, 2])
    path = os.path.join(ROOT, "tests", "golden", "coaxial_matched.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
