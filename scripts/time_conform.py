"""What the conforming prolongation of a hanging-node space costs: an O-grid cylinder of about --elements elements at order 3,
the elements inside a ball that holds about --fraction of them refined once (fem/nchex.py).  Timed in one process, the two
forms alternating, device events after warm-up:
  * ParOperator::Mult with the constraint (masked P, local apply, P^T with the essential rows: three launches);
  * ParOperator::Mult of the SAME local operator wrapped with n_true = n_local and no constraint -- the fused single-launch
    path every conforming space takes;
  * the two kernels of pa_conform.hip alone;
  * PCG + p-multigrid (orders 1, 2, 3; Chebyshev smoothing, Jacobi-PCG at level 0) iterations per second on both: the
    constrained hierarchy loses the smoother step fused into the operator, the unconstrained one keeps it.
Writes profiles/r16_conform.json (or --out)."""
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
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pcg-its", type=int, default=30)
    ap.add_argument("--host-only", action="store_true", help="build the mesh and the spaces, print their sizes, stop")
    ap.add_argument("--out", default=os.path.join("profiles", "r16_conform.json"))
    args = ap.parse_args()

    from palace_amd.fem import nchex
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.fem.mesh import ogrid_cylinder

    p = args.order
    n = max(1, int(round((args.elements / (5 * 1.2)) ** (1.0 / 3.0))))
    nz = max(1, int(round(args.elements / (5 * n * n))))
    t0 = time.perf_counter()
    m0 = ogrid_cylinder(n, nz)
    ctr = m0.x[m0.elem_nodes[:, 13]]                                    # element centres (the middle lattice node)
    lo, hi = m0.bounding_box()
    d = np.linalg.norm(ctr - 0.5 * (lo + hi) - np.array([0.3, 0.2, 0.1]) * (hi - lo), axis=1)
    marked = np.argsort(d, kind="stable")[: int(round(args.fraction * m0.ne))]
    mesh = nchex.refine_local(m0, marked)
    levels = list(range(1, p + 1))
    spaces = [nchex.NCSpace(NDHexSpace(mesh, q)) for q in levels]
    s = spaces[-1]
    t_host = time.perf_counter() - t0
    res = dict(elements_start=int(m0.ne), elements=int(mesh.ne), refined=int(mesh.marked.size), order=p, n_local=int(s.n_local),
               n_true=int(s.n_true), constrained_share=float((s.n_local - s.n_true) / s.n_local), nnz_C=int(s.C.nnz),
               longest_row=int(np.diff(s.C.indptr).max()), longest_row_T=int(np.diff(s.C.tocsc().indptr).max()),
               host_setup_s=round(t_host, 1))
    print(res, flush=True)
    if args.host_only:
        return

    import torch

    from palace_amd import ceed, linalg
    from tests import util

    ctx = linalg.Context()
    cm, bm = util.make_ctx("scalar")
    cc, bc = util.make_ctx("identity")
    geom = ceed.GeomFactorData(mesh, p + 1)
    fine = ceed.curlcurlmass_operator(geom, s, bm, bc)
    local = [fine.coarsen(geom, q) for q in spaces[:-1]] + [fine]
    conf = [linalg.Conforming(ctx, q) for q in spaces]
    ess_local = [NDHexSpace.ess_dofs(q) for q in spaces]                  # every boundary dof of the broken space
    A_c = [linalg.ParOperator(ctx, op, q.ess_dofs(), linalg.DIAG_ONE, conforming=c) for op, q, c in zip(local, spaces, conf)]
    A_u = [linalg.ParOperator(ctx, op, e, linalg.DIAG_ONE) for op, e in zip(local, ess_local)]
    res["lanes"], res["lanes_T"] = conf[-1].lanes(), conf[-1].lanes(True)
    res["unconstrained_fuses_essential"] = A_u[-1].fuses_essential()

    def new(k):
        return torch.rand(k, dtype=torch.float64, device="cuda")

    xt, yt, xl, yl = new(s.n_true), new(s.n_true), new(s.n_local), new(s.n_local)
    mask = torch.zeros(s.n_true, dtype=torch.uint8, device="cuda")
    mask[torch.from_numpy(s.ess_dofs().astype(np.int64)).cuda()] = 1
    forms = {
        "mult_constrained": lambda: A_c[-1].mult(xt, yt),
        "mult_unconstrained": lambda: A_u[-1].mult(xl, yl),
        "prolongate": lambda: conf[-1].prolongate(xt, xl, mask),
        "restrict": lambda: conf[-1].restrict(yl, yt, conf[-1].FIX_ONE, 1.0, mask, xt),
        "local_apply": lambda: fine.mult(xl, yl),
    }
    for f in forms.values():
        for _ in range(20):
            f()
    times = {k: [] for k in forms}
    with torch.cuda.stream(ctx.torch_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):                                                # the forms alternate: five rounds each
            for k, f in forms.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.reps * 1e3)
    res["us"] = {k: dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()}
    print(res["us"], flush=True)

    def pcg(A, P, nt):
        coarse = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1e-3, max_it=200)
        B = linalg.gmg(ctx, A, P, coarse, cheby_order=4)
        K = linalg.cg(ctx, A[-1], B, rel_tol=1e-30, max_it=args.pcg_its)
        fused = [bool(B.fused_step(l)) for l in range(1, len(A))]
        return K, fused, (coarse, B)

    P_c = [linalg.Interp(ctx, a, b, conforming=c) for a, b, c in zip(spaces[:-1], spaces[1:], conf[:-1])]
    P_u = [linalg.Interp(ctx, a, b, n_true_c=a.n_local, n_true_f=b.n_local) for a, b in zip(spaces[:-1], spaces[1:])]
    solvers = {"constrained": pcg(A_c, P_c, s.n_true) + (s.n_true, s.ess_dofs()),
               "unconstrained": pcg(A_u, P_u, s.n_local) + (s.n_local, ess_local[-1])}
    its = {k: [] for k in solvers}
    state = {}
    for k, (K, fused, keep, nt, ess) in solvers.items():
        b = new(nt) - 0.5
        b[torch.from_numpy(np.asarray(ess).astype(np.int64)).cuda()] = 0.0
        x = torch.zeros(nt, dtype=torch.float64, device="cuda")
        K.mult(b, x), K.mult(b, x)                                        # direct run, then the recording
        state[k] = (b, x)
    for _ in range(3):
        for k, (K, fused, keep, nt, ess) in solvers.items():
            b, x = state[k]
            torch.cuda.synchronize()
            t = time.perf_counter()
            K.mult(b, x)
            torch.cuda.synchronize()
            its[k].append(K.stats()["iterations"] / (time.perf_counter() - t))
    res["pcg_it_per_s"] = {k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1),
                                   smoother_steps_fused=solvers[k][1]) for k, v in its.items()}
    print(res["pcg_it_per_s"], flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
