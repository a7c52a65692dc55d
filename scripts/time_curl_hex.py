"""Discrete curl ND(p) -> RT(p) on the bench-size cylinder (cylinder_for_dofs(10e6, 3)) at p = 2, 3 and 4: C and C^T on the
sum-factorised tensor form (pa_curl_hex.hip behind linalg.Curl) and on the dense interpolator with rthex.hex_curl_matrix
(linalg.DenseInterp), timed alternately in one process, PAIRS times each, so that the run-to-run spread is visible.  At p = 4
the dense interpolator cannot be created (300 Nedelec dofs per element, it stops at 256): the line says so and carries the
tensor times alone.  The bytes are the necessary traffic computed from the shapes: 4 (P_ND + P_RT) of index per element, 8 per
Nedelec dof and 8 per Raviart-Thomas dof (one side read, the other written); bytes over time is a WHOLE-OPERATOR rate against
the 6.29 TB/s copy rate -- the forward kernel alone for C, kernel plus gather for C^T (whose E-vector traffic is not counted).
One JSON line per order.
  python scripts/time_curl_hex.py            (PAIRS=5 REPS=30 DOFS=10.0e6 ORDERS=2,3,4)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import lib as _lib  # noqa: E402
from palace_amd import linalg  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import cylinder_for_dofs  # noqa: E402

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


ctx = linalg.Context()
mesh = cylinder_for_dofs(float(os.environ.get("DOFS", "10.0e6")), 3)
orders = [int(v) for v in os.environ.get("ORDERS", "2,3,4").split(",")]

for p in orders:
    nd, rt = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p)
    tensor = linalg.Curl(ctx, nd, rt)
    dom = dict(offsets=nd.elem_dof_lex, lsize=nd.ndofs, orients=nd.elem_sign_lex < 0)
    try:
        dense = linalg.DenseInterp(ctx, dom, rt.restriction(interp_range=True), rthex.hex_curl_matrix(p))
        dense_error = None
    except _lib.PalaceAmdError as e:  # (more than 256 dofs per element on either side)
        dense, dense_error = None, str(e)
    gen = torch.Generator(device="cuda").manual_seed(12)
    a = torch.rand(nd.ndofs, dtype=torch.float64, device="cuda", generator=gen)
    b = torch.rand(rt.ndofs, dtype=torch.float64, device="cuda", generator=gen)
    bt, bd, at, ad = torch.empty_like(b), torch.empty_like(b), torch.empty_like(a), torch.empty_like(a)
    ms = {"tensor_C": [], "tensor_Ct": [], "dense_C": [], "dense_Ct": []}
    for _ in range(PAIRS):
        ms["tensor_C"].append(timed(ctx, lambda: tensor.mult(a, bt), 5, REPS))
        if dense is not None:
            ms["dense_C"].append(timed(ctx, lambda: dense.mult(a, bd), 5, REPS))
        ms["tensor_Ct"].append(timed(ctx, lambda: tensor.mult_transpose(b, at), 5, REPS))
        if dense is not None:
            ms["dense_Ct"].append(timed(ctx, lambda: dense.mult_transpose(b, ad), 5, REPS))
    nbytes = int(mesh.ne) * 4 * (nd.P + rt.P) + 8 * nd.ndofs + 8 * rt.ndofs
    out = {"workload": f"discrete curl ND -> RT p={p}, {mesh.ne} hexahedra, {nd.ndofs} ND dofs, {rt.ndofs} RT dofs",
           "p": p, "nd_dofs": nd.ndofs, "rt_dofs": rt.ndofs, "elements": int(mesh.ne), "pairs": PAIRS, "reps": REPS,
           "necessary_bytes": nbytes}
    for d in ("C", "Ct"):
        t = ms["tensor_" + d]
        out[f"tensor_{d}_ms"] = t
        out[f"tensor_{d}_ms_median"] = float(np.median(t))
        out[f"tensor_{d}_spread"] = (max(t) - min(t)) / float(np.median(t))
        out[f"tensor_{d}_whole_operator_TBps"] = nbytes / (float(np.median(t)) * 1e-3) / 1e12
        out[f"tensor_{d}_fraction_of_copy_rate"] = out[f"tensor_{d}_whole_operator_TBps"] / COPY_TBPS
        if dense is not None:
            dn = ms["dense_" + d]
            out[f"dense_{d}_ms"] = dn
            out[f"dense_{d}_ms_median"] = float(np.median(dn))
            out[f"dense_{d}_spread"] = (max(dn) - min(dn)) / float(np.median(dn))
            out[f"speedup_{d}_median"] = float(np.median(dn) / np.median(t))
            out[f"tensor_{d}_faster_beyond_spread"] = bool(max(t) < min(dn))
    if dense is not None:
        out["max_rel_diff_C"] = float((bt - bd).abs().max() / bd.abs().max())
        out["max_rel_diff_Ct"] = float((at - ad).abs().max() / ad.abs().max())
    else:
        out["dense_unavailable"] = dense_error
    print(json.dumps(out), flush=True)
    del tensor, dense
    torch.cuda.empty_cache()
