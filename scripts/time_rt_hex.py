"""Raviart-Thomas mass on the bench-size cylinder (cylinder_for_dofs(10e6, 3)) with the rotated sapphire tensor of
bench_legs/hex.py, at (p, q1d) = (2, 3), (3, 4) and (4, 5): Operator::Mult on the sum-factorised tensor path (pa_rt_hex.hip) and
on the dense-table path (pa_dense.hip), timed alternately in one process, PAIRS times each, so that the run-to-run spread is
visible; pa_op_algorithmic_bytes of the tensor operator over its time as a fraction of the 6.29 TB/s copy rate; at (3, 4) also
PCG + Jacobi iterations per second on both paths.  Where the dense path has no instantiation for the element (more than 144 dofs: RT p = 4)
the line says so and carries the tensor time alone.  One JSON line per pair of orders.
  python scripts/time_rt_hex.py            (PAIRS=5 REPS=30 DOFS=10.0e6 PQ=2:3,3:4,4:5)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.basis1d import gauss_legendre  # noqa: E402
from palace_amd.fem.mesh import _q2_1d, cylinder_for_dofs  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", "5"))
REPS = int(os.environ.get("REPS", "30"))
COPY_TBPS = 6.29


def timed(ctx, fn, warm, reps):
    for _ in range(warm):
        fn()
    with torch.cuda.stream(ctx.torch_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def q2_grad_table(q1d):
    """Gradient table [3, Q, 27] of the tri-quadratic mesh-node basis at the tensor Gauss-Legendre points, and the weights [Q]."""
    x, w = gauss_legendre(q1d)
    B, G = _q2_1d(x)
    T = np.stack([np.einsum("ck,bj,ai->cbakji", B, B, G), np.einsum("ck,bj,ai->cbakji", B, G, B),
                  np.einsum("ck,bj,ai->cbakji", G, B, B)]).reshape(3, q1d ** 3, 27)
    return T, np.einsum("c,b,a->cba", w, w, w).ravel()


ctx = linalg.Context()
mesh = cylinder_for_dofs(float(os.environ.get("DOFS", "10.0e6")), 3)
c, s_ = np.cos(0.3), np.sin(0.3)
R = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s_], [0.0, s_, c]])
eps = R @ np.diag([9.3, 9.3, 11.5]) @ R.T
eps = 0.5 * (eps + eps.T)  # (exactly symmetric: the packed form is chosen on an exact test)
blob = ceed.coefficient_context(3, attr_mat=[0] * int(mesh.attr.max()), mat_coeff=[eps])
pairs = [tuple(int(v) for v in t.split(":")) for t in os.environ.get("PQ", "2:3,3:4,4:5").split(",")]

for p, q1d in pairs:
    sp = rthex.RTHexSpace(mesh, p)
    n = sp.ndofs
    tensor = ceed.rtmass_operator(ceed.GeomFactorData(mesh, q1d), sp, blob)
    grad, wts = q2_grad_table(q1d)
    dgeom = ceed.DenseGeomFactorData(mesh.elem_nodes, mesh.x, mesh.attr, grad, wts)
    rint, _ = rthex.rt_hex_tables(p, gauss_legendre(q1d)[0])
    block = ceed.DenseBlock(ceed.FE_HDIV, n, sp.elem_dof_lex, rint, None, orients=sp.elem_sign_lex < 0)
    try:
        dense = ceed.Operator(n, n).add_dense_integrator(dgeom, block, ceed.QF_HDIV_33, blob, ceed.EVAL_INTERP).finalize()
        dense_error = None
    except ceed._lib.PalaceAmdError as e:  # (the dense path is instantiated up to 144 dofs per element: RT p = 4 has 240)
        dense, dense_error = None, str(e)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    yt, yd = torch.empty_like(x), torch.empty_like(x)
    t_ms, d_ms = [], []
    for _ in range(PAIRS):
        t_ms.append(timed(ctx, lambda: tensor.mult(x, yt), 5, REPS))
        if dense is not None:
            d_ms.append(timed(ctx, lambda: dense.mult(x, yd), 5, REPS))
    out = {"workload": f"RT mass p={p} q1d={q1d}, {mesh.ne} hexahedra, {n} dofs, rotated sapphire tensor",
           "p": p, "q1d": q1d, "dofs": n, "elements": int(mesh.ne), "pairs": PAIRS, "reps": REPS,
           "tensor_ms": t_ms, "tensor_ms_median": float(np.median(t_ms)),
           "tensor_spread": (max(t_ms) - min(t_ms)) / float(np.median(t_ms))}
    if dense is not None:
        out.update({"dense_ms": d_ms, "dense_ms_median": float(np.median(d_ms)),
                    "dense_spread": (max(d_ms) - min(d_ms)) / float(np.median(d_ms)),
                    "speedup_median": float(np.median(d_ms) / np.median(t_ms)),
                    "tensor_faster_beyond_spread": bool(max(t_ms) < min(d_ms)),
                    "max_rel_diff": float((yt - yd).abs().max() / yd.abs().max())})
    else:
        out["dense_unavailable"] = dense_error
    nbytes = tensor.algorithmic_bytes()
    out["algorithmic_bytes"] = nbytes
    out["algorithmic_TBps"] = nbytes / (out["tensor_ms_median"] * 1e-3) / 1e12
    out["fraction_of_copy_rate"] = out["algorithmic_TBps"] / COPY_TBPS
    if (p, q1d) == (3, 4):  # the solve the kernel exists for: a fixed number of PCG + Jacobi iterations
        its = 50
        for name, op in (("tensor", tensor), ("dense", dense)):
            if op is None:
                continue
            M = linalg.ParOperator(ctx, op, np.zeros(0, dtype=np.int32))
            solver = linalg.cg(ctx, M, linalg.jacobi(ctx, M), rel_tol=0.0, max_it=its)
            b, d = torch.empty_like(x), torch.empty_like(x)
            M.mult(x, b)

            def solve():
                d.zero_()
                solver.mult(b, d)

            ms = timed(ctx, solve, 1, 3)
            out[f"pcg_jacobi_{name}_iterations_per_s"] = solver.stats()["iterations"] / (ms * 1e-3)
    print(json.dumps(out), flush=True)
    del tensor, dense, dgeom, block
    torch.cuda.empty_cache()
