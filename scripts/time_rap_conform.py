"""What the assembled level 0 of a hanging-node hierarchy costs and buys: the refined O-grid cylinder of scripts/time_conform.py
(about --elements elements, the ones inside a ball that holds about --fraction of them refined once), Nedelec K + M, level 0 at
order 1.  One process, after warm-up:
  1. the device triple product P^T A P (pa_rap_conform.hip), symbolic and numeric phase separately, against the host route a
     caller needed before it existed: copy the local matrix back, two sparse products on the host (scipy), upload;
  2. the level-0 Mult as ONE sparse product on the assembled true-dof matrix against the three launches (masked P, partially
     assembled local apply, P^T with the essential rows) of the constrained operator on the same level, alternating;
  3. PCG + p-multigrid [1 .. --order] with AMS on the assembled level 0 (true-dof gradient from the injection-form product)
     against the Jacobi-PCG level 0 on the three-launch operator: iterations to 1e-8 and iterations per second.
Writes profiles/r17_rap_conform.json (or --out)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=float, default=1e5)
    ap.add_argument("--fraction", type=float, default=0.10)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "r17_rap_conform.json"))
    args = ap.parse_args()

    from palace_amd.fem import nchex
    from palace_amd.fem.fespace import H1HexSpace, NDHexSpace, vertex_coordinates
    from palace_amd.fem.mesh import ogrid_cylinder

    n = max(1, int(round((args.elements / (5 * 1.2)) ** (1.0 / 3.0))))
    nz = max(1, int(round(args.elements / (5 * n * n))))
    m0 = ogrid_cylinder(n, nz)
    ctr = m0.x[m0.elem_nodes[:, 13]]
    lo, hi = m0.bounding_box()
    d = np.linalg.norm(ctr - 0.5 * (lo + hi) - np.array([0.3, 0.2, 0.1]) * (hi - lo), axis=1)
    mesh = nchex.refine_local(m0, np.argsort(d, kind="stable")[: int(round(args.fraction * m0.ne))])
    spaces = [nchex.NCSpace(NDHexSpace(mesh, q)) for q in range(1, args.order + 1)]
    h1 = nchex.NCSpace(H1HexSpace(mesh, 1))
    s0 = spaces[0]
    res = dict(elements=int(mesh.ne), orders=[s.p for s in spaces], level0_n_local=int(s0.n_local), level0_n_true=int(s0.n_true),
               fine_n_true=int(spaces[-1].n_true))
    print(res, flush=True)

    import torch

    from palace_amd import ceed, linalg
    from tests import nc_util, util

    ctx = linalg.Context()
    bm, bc = util.make_ctx("scalar")[1], util.make_ctx("identity")[1]
    geom = ceed.GeomFactorData(mesh, args.order + 1)
    fine = ceed.curlcurlmass_operator(geom, spaces[-1], bm, bc)
    local = [fine.coarsen(geom, q) for q in spaces[:-1]] + [fine]
    conf = [linalg.Conforming(ctx, q) for q in spaces]
    A = [linalg.ParOperator(ctx, op, q.ess_dofs(), linalg.DIAG_ONE, conforming=c) for op, q, c in zip(local, spaces, conf)]
    P = [linalg.Interp(ctx, a, b, conforming=c) for a, b, c in zip(spaces[:-1], spaces[1:], conf[:-1])]

    # ---- 1. the product
    B = local[0].full_assemble_device()
    res["local_nnz"] = int(B.nnz)
    for _ in range(2):
        T = linalg.rap_conforming(ctx, B, conf[0], conf[0])
    sym, num = [], []
    for _ in range(7):
        t = []
        T = linalg.rap_conforming(ctx, B, conf[0], conf[0], timings=t)
        sym.append(t[0]), num.append(t[1])
    res["product_nnz"] = int(T.nnz)
    Pm = s0.prolongation()
    host = dict(download=[], multiply=[], upload=[])
    for _ in range(3):
        t0 = time.perf_counter()
        Bh = B.to_scipy()
        t1 = time.perf_counter()
        Th = (Pm.T @ Bh @ Pm).tocsr()
        Th.sort_indices()
        t2 = time.perf_counter()
        Tu = ceed.DeviceCsr.from_scipy(Th, symmetric=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        host["download"].append((t1 - t0) * 1e3), host["multiply"].append((t2 - t1) * 1e3), host["upload"].append((t3 - t2) * 1e3)
    got = T.to_scipy()
    res["product_vs_host_relmax"] = float(abs(got - Th).max() / abs(Th).max())
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    res["product_ms"] = dict(device_symbolic=med(sym), device_numeric=med(num), device_total=med(np.add(sym, num)),
                             host_download=med(host["download"]), host_multiply_scipy=med(host["multiply"]), host_upload=med(host["upload"]),
                             host_total=med(np.sum([host[k] for k in host], axis=0)), all_device_symbolic=[round(v, 3) for v in sym],
                             all_device_numeric=[round(v, 3) for v in num])
    print(res["product_ms"], flush=True)

    # ---- 2. the level-0 Mult
    ess0 = s0.ess_dofs()
    A0 = linalg.AssembledParOperator(ctx, T, ess0, linalg.DIAG_ONE)
    x, y = torch.rand(s0.n_true, dtype=torch.float64, device="cuda"), torch.zeros(s0.n_true, dtype=torch.float64, device="cuda")
    forms = {"assembled_spmv": lambda: A0.mult(x, y), "three_launches": lambda: A[0].mult(x, y)}
    ya = A0.mult(x, torch.zeros_like(y)).clone()
    yb = A[0].mult(x, torch.zeros_like(y)).clone()
    res["level0_mult_relmax"] = float((ya - yb).abs().max() / yb.abs().max())
    for f in forms.values():
        for _ in range(20):
            f()
    times = {k: [] for k in forms}
    with torch.cuda.stream(ctx.torch_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            for k, f in forms.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.reps * 1e3)
    res["level0_mult_us"] = {k: dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()}
    print(res["level0_mult_us"], flush=True)

    # ---- 3. PCG + p-multigrid
    if len(spaces) > 1:
        t0 = time.perf_counter()
        Gl = nc_util.local_gradient(h1, s0)
        G = linalg.rap_conforming(ctx, ceed.DeviceCsr.from_scipy(Gl), test=conf[0], trial=linalg.Conforming(ctx, h1), injection=True).to_scipy()
        ams = linalg.ams(ctx, T, ess0, G, vertex_coordinates(h1)[: h1.n_true])
        torch.cuda.synchronize()
        res["ams_setup_s"] = round(time.perf_counter() - t0, 2)
        pcg0 = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1e-2, max_it=8)
        nt, ess = spaces[-1].n_true, spaces[-1].ess_dofs()
        b = A[-1].mult(torch.ones(nt, dtype=torch.float64, device="cuda"), torch.zeros(nt, dtype=torch.float64, device="cuda"))
        b[torch.from_numpy(ess.astype(np.int64)).cuda()] = 0.0
        solvers = {"ams_assembled_level0": linalg.gmg(ctx, [A0] + A[1:], P, ams, cheby_order=4),
                   "jacobi_pcg_level0": linalg.gmg(ctx, A, P, pcg0, cheby_order=4)}
        out = {}
        for k, Bk in solvers.items():
            K = linalg.cg(ctx, A[-1], Bk, rel_tol=1e-8, max_it=400)
            xs = torch.zeros_like(b)
            K.mult(b, xs), K.mult(b, xs)                                   # direct run, then the recording
            rate = []
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                K.mult(b, xs)
                torch.cuda.synchronize()
                rate.append(K.stats()["iterations"] / (time.perf_counter() - t))
            out[k] = dict(iterations=int(K.stats()["iterations"]), converged=bool(K.stats()["converged"]),
                          it_per_s=dict(median=round(float(np.median(rate)), 1), min=round(min(rate), 1), max=round(max(rate), 1)))
        res["pcg"] = out
        print(out, flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
