"""The two-space forms of the flux error estimators on the bench-size cylinder (cylinder_for_dofs(10e6, 3)) with the rotated
sapphire tensor of bench_legs/hex.py, at (p, q1d) = (2, 3), (3, 4) and (4, 5): both directions of the mixed mass (v, C u) between
the Nedelec and the Raviart-Thomas space and the element error integrator, on the sum-factorised tensor path (pa_mixed_hex.hip)
and on the dense two-space path (pa_mixed.hip), timed alternately in one process, PAIRS times each, so that the run-to-run
spread is visible.  The tensor form counts as faster only where every one of its times is below every dense time.  Where the
dense descriptors cannot be created for the element the line says so and carries the tensor times alone.  Bytes over time: for
the mixed mass pa_op_algorithmic_bytes, for the error integrator the same count with both vectors read and one double per element
written.  One JSON line per form and pair of orders.
  python scripts/time_mixed_hex.py            (PAIRS=5 REPS=30 DOFS=10.0e6 PQ=2:3,3:4,4:5)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.basis1d import gauss_legendre  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
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


def nd_dense_tables(nd, q1d):
    """(values, curls) [3, Q, P] of the Nedelec element in its native order."""
    from oracle import palace_oracle as po

    nint, ncurl = po.nd_hex_dense_tables(nd.p, q1d, nd.dof_map_native())
    return np.asarray(nint).reshape(3, -1, nd.P), np.asarray(ncurl).reshape(3, -1, nd.P)


ctx = linalg.Context()
mesh = cylinder_for_dofs(float(os.environ.get("DOFS", "10.0e6")), 3)
c, s_ = np.cos(0.3), np.sin(0.3)
R = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s_], [0.0, s_, c]])
eps = R @ np.diag([9.3, 9.3, 11.5]) @ R.T
eps = 0.5 * (eps + eps.T)
w_, V_ = np.linalg.eigh(eps)
nattr = int(mesh.attr.max())
blob = ceed.coefficient_context(3, attr_mat=[0] * nattr, mat_coeff=[eps])
pair = np.concatenate([ceed.coefficient_context(3, attr_mat=[0] * nattr, mat_coeff=[(V_ * np.sqrt(w_)) @ V_.T]),
                       ceed.coefficient_context(3, attr_mat=[0] * nattr, mat_coeff=[(V_ / np.sqrt(w_)) @ V_.T])])
pairs = [tuple(int(v) for v in t.split(":")) for t in os.environ.get("PQ", "2:3,3:4,4:5").split(",")]


def report(form, p, q1d, nd, sp, t_ms, d_ms, dense_error, nbytes, diff):
    out = {"workload": f"{form} p={p} q1d={q1d}, {mesh.ne} hexahedra, ND {nd.ndofs} / RT {sp.ndofs} dofs, rotated sapphire tensor",
           "form": form, "p": p, "q1d": q1d, "elements": int(mesh.ne), "pairs": PAIRS, "reps": REPS,
           "tensor_ms": t_ms, "tensor_ms_median": float(np.median(t_ms)),
           "tensor_spread": (max(t_ms) - min(t_ms)) / float(np.median(t_ms))}
    if d_ms:
        out.update({"dense_ms": d_ms, "dense_ms_median": float(np.median(d_ms)),
                    "dense_spread": (max(d_ms) - min(d_ms)) / float(np.median(d_ms)),
                    "speedup_median": float(np.median(d_ms) / np.median(t_ms)),
                    "tensor_faster_beyond_spread": bool(max(t_ms) < min(d_ms)), "max_rel_diff": diff})
    else:
        out["dense_unavailable"] = dense_error
    out["algorithmic_bytes"] = nbytes
    out["algorithmic_TBps"] = nbytes / (out["tensor_ms_median"] * 1e-3) / 1e12
    out["fraction_of_copy_rate"] = out["algorithmic_TBps"] / COPY_TBPS
    print(json.dumps(out), flush=True)


for p, q1d in pairs:
    nd, sp = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, q1d)
    grad, wts = q2_grad_table(q1d)
    dgeom = ceed.DenseGeomFactorData(mesh.elem_nodes, mesh.x, mesh.attr, grad, wts)
    off, ori = nd.native_restriction()
    nint, ncurl = nd_dense_tables(nd, q1d)
    rint, _ = rthex.rt_hex_tables(p, gauss_legendre(q1d)[0])
    ndb = ceed.DenseBlock(ceed.FE_HCURL, nd.ndofs, off, nint, ncurl, orients=ori)
    rtb = ceed.DenseBlock(ceed.FE_HDIV, sp.ndofs, sp.elem_dof_lex, rint, None, orients=sp.elem_sign_lex < 0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    xs = {id(nd): torch.rand(nd.ndofs, dtype=torch.float64, device="cuda", generator=gen),
          id(sp): torch.rand(sp.ndofs, dtype=torch.float64, device="cuda", generator=gen)}
    for form, (s1, d1), (s2, d2), qf, qfe in (("mixed mass ND->RT", (nd, ndb), (sp, rtb), ceed.QF_HCURLHDIV_33, ceed.QF_HCURLHDIV_ERROR_33),
                                              ("mixed mass RT->ND", (sp, rtb), (nd, ndb), ceed.QF_HDIVHCURL_33, ceed.QF_HDIVHCURL_ERROR_33)):
        tensor = ceed.mixedmass_operator(geom, s1, s2, blob)
        try:
            dense = ceed.Operator(d2.lsize, d1.lsize).add_dense_mixed_integrator(dgeom, d1, d2, qf, blob).finalize()
            dense_error = None
        except ceed._lib.PalaceAmdError as e:
            dense, dense_error = None, str(e)
        x = xs[id(s1)]
        yt, yd = torch.empty(s2.ndofs, dtype=torch.float64, device="cuda"), torch.empty(s2.ndofs, dtype=torch.float64, device="cuda")
        t_ms, d_ms = [], []
        for _ in range(PAIRS):
            t_ms.append(timed(ctx, lambda: tensor.mult(x, yt), 5, REPS))
            if dense is not None:
                try:
                    d_ms.append(timed(ctx, lambda: dense.mult(x, yd), 5, REPS))
                except ceed._lib.PalaceAmdError as e:  # (the dense kernel's LDS limit shows at the first apply)
                    dense, dense_error = None, str(e)
        diff = float((yt - yd).abs().max() / yd.abs().max()) if d_ms else None
        report(form, p, q1d, nd, sp, t_ms, d_ms, dense_error, tensor.algorithmic_bytes(), diff)
        del tensor, dense
    # the element error integrator (first input Nedelec: GradFluxErrorEstimator's)
    tensor = ceed.HexElementErrorIntegrator(geom, nd, sp, ceed.QF_HCURLHDIV_ERROR_33, pair)
    try:
        dense = ceed.ElementErrorIntegrator(dgeom, ndb, rtb, ceed.QF_HCURLHDIV_ERROR_33, pair)
        dense_error = None
    except ceed._lib.PalaceAmdError as e:
        dense, dense_error = None, str(e)
    et, ed = torch.zeros(mesh.ne, dtype=torch.float64, device="cuda"), torch.zeros(mesh.ne, dtype=torch.float64, device="cuda")
    t_ms, d_ms = [], []
    for _ in range(PAIRS):
        t_ms.append(timed(ctx, lambda: tensor.apply_add(xs[id(nd)], xs[id(sp)], et), 5, REPS))
        if dense is not None:
            try:
                d_ms.append(timed(ctx, lambda: dense.apply_add(xs[id(nd)], xs[id(sp)], ed), 5, REPS))
            except ceed._lib.PalaceAmdError as e:
                dense, dense_error = None, str(e)
    diff = float((et / et.max() - ed / ed.max()).abs().max()) if d_ms else None  # (both accumulated the same number of applies)
    nbytes = mesh.ne * (q1d ** 3 * 11 * 8 + (nd.P + sp.P) * 6 + 8) + 8.0 * (nd.ndofs + sp.ndofs)
    report("element error ND, RT", p, q1d, nd, sp, t_ms, d_ms, dense_error, nbytes, diff)
    del tensor, dense, dgeom, ndb, rtb, geom
    torch.cuda.empty_cache()
