"""Writes the arrays examples/cxx_host/estimate_nc.cpp reads: a locally refined hexahedral mesh with hanging nodes (mesh A or C
of tests/nc_util.py), the constrained Nedelec and Raviart-Thomas spaces of order p on it (fem/nchex.py: NCSpace; tensor
descriptions with the true dofs first, and the constraint rows C of either space in CSR), two materials each for the permittivity
and the inverse permeability, and complex fields E (H(curl)) and B (H(div)) on the true dofs.
    python dump_estimator_nc_problem.py problem.bin [mesh] [p]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dump_estimator_hex_problem as ep  # noqa: E402
from palace_amd.fem import nchex, rthex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402

_cache = {}


def problem(name="C", p=2):
    if (name, p) not in _cache:
        from tests import nc_util as nu

        mesh = nu.nc_mesh(name)
        assert set(np.unique(mesh.attr).tolist()) <= {1, 2}
        nd, rt = nchex.NCSpace(NDHexSpace(mesh, p)), nchex.NCSpace(rthex.RTHexSpace(mesh, p))
        rng = np.random.default_rng(60 + p)
        _cache[name, p] = dict(mesh=mesh, nd=nd, rt=rt, p=p, q1d=p + 1, eps=ep.EPS, muinv=ep.MUINV,
                               E=rng.uniform(-1, 1, nd.n_true), E_im=rng.uniform(-1, 1, nd.n_true),
                               B=rng.uniform(-1, 1, rt.n_true), B_im=rng.uniform(-1, 1, rt.n_true))
    return _cache[name, p]


def _csr(space):
    return [space.C.indptr.astype(np.int32), space.C.indices.astype(np.int32), space.C.data.astype(np.float64)]


def main(path, name="C", p=2):
    P = problem(name, int(p))
    mesh, nd, rt = P["mesh"], P["nd"], P["rt"]
    arrays = [np.array([mesh.ne, mesh.x.shape[0], P["p"], P["q1d"], nd.n_local, rt.n_local, nd.n_true, rt.n_true], dtype=np.int32),
              mesh.elem_nodes.astype(np.int32), mesh.x.astype(np.float64), mesh.attr.astype(np.int32),
              nd.elem_dof_lex.astype(np.int32), (nd.elem_sign_lex < 0).astype(np.uint8),
              rt.elem_dof_lex.astype(np.int32), (rt.elem_sign_lex < 0).astype(np.uint8),
              np.concatenate([e.T.ravel() for e in P["eps"]]), np.concatenate([m.T.ravel() for m in P["muinv"]]),
              *_csr(nd), *_csr(rt), P["E"], P["E_im"], P["B"], P["B_im"]]
    with open(path, "wb") as f:
        f.write(np.array([len(arrays)], dtype=np.int64).tobytes())
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(np.array([a.nbytes], dtype=np.int64).tobytes())
            f.write(a.tobytes())


if __name__ == "__main__":
    main(*sys.argv[1:])
