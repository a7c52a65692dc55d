"""What the estimator pass on a hanging-node mesh costs: the refined cylinder of scripts/time_conform.py (an O-grid cylinder of
about --elements elements, the elements inside a ball that holds about --fraction of them refined once) at order 3, constrained
Nedelec and Raviart-Thomas spaces (fem/nchex.py).  Timed in one process, the forms alternating, device events after warm-up:
  * Conforming.prolongate2 / restrict2 against two one-vector launches (the Nedelec constraint);
  * the complex mass apply of the flux projector as P2, Mult2, P^T2 (three launches) against ComplexParOperator.mult (two real
    ParOperators: six launches), on the Nedelec mass (curl-flux) and on the Raviart-Thomas mass (grad-flux);
  * one full curl-flux estimate (P, flux, P^T, PCG + Jacobi on P^T M P to 1e-13, P, element integrator) on the constrained mesh
    against the same estimate on the unrefined mesh without constraints, per element.
Writes profiles/r18_nc_estimator.json (or --out)."""
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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-only", action="store_true", help="build the mesh and the spaces, print their sizes, stop")
    ap.add_argument("--out", default=os.path.join("profiles", "r18_nc_estimator.json"))
    args = ap.parse_args()

    from palace_amd.fem import nchex, rthex
    from palace_amd.fem.fespace import NDHexSpace
    from palace_amd.fem.mesh import ogrid_cylinder

    p = args.order
    n = max(1, int(round((args.elements / (5 * 1.2)) ** (1.0 / 3.0))))
    nz = max(1, int(round(args.elements / (5 * n * n))))
    t0 = time.perf_counter()
    m0 = ogrid_cylinder(n, nz)
    ctr = m0.x[m0.elem_nodes[:, 13]]
    lo, hi = m0.bounding_box()
    d = np.linalg.norm(ctr - 0.5 * (lo + hi) - np.array([0.3, 0.2, 0.1]) * (hi - lo), axis=1)
    marked = np.argsort(d, kind="stable")[: int(round(args.fraction * m0.ne))]
    mesh = nchex.refine_local(m0, marked)
    nd, rt = nchex.NCSpace(NDHexSpace(mesh, p)), nchex.NCSpace(rthex.RTHexSpace(mesh, p))
    nd0, rt0 = NDHexSpace(m0, p), rthex.RTHexSpace(m0, p)
    res = dict(elements_start=int(m0.ne), elements=int(mesh.ne), refined=int(mesh.marked.size), order=p,
               nd=dict(n_local=int(nd.n_local), n_true=int(nd.n_true), nnz_C=int(nd.C.nnz)),
               rt=dict(n_local=int(rt.n_local), n_true=int(rt.n_true), nnz_C=int(rt.C.nnz)),
               host_setup_s=round(time.perf_counter() - t0, 1))
    print(res, flush=True)
    if args.host_only:
        return

    import torch

    from oracle import palace_oracle as po
    from palace_amd import ceed, linalg
    from tests import test_mixed_hex_gpu as mh
    from tests.test_nc_estimator_gpu import NCEstimator

    ctx = linalg.Context()

    def new(k):
        return torch.rand(k, dtype=torch.float64, device="cuda") - 0.5

    est_c = NCEstimator(ctx, nd, rt, "curl", [np.eye(3)])                 # the pieces on the constrained mesh
    geom = est_c.geom
    c_nd, c_rt = est_c.c_sm, est_c.c_rhs
    nd_mass, rt_mass = est_c.mass, ceed.rtmass_operator(geom, rt, po.CoeffCtx().pack())
    res["nd_mass"] = dict(two_rhs=nd_mass.two_rhs(), streams=nd_mass.streams())
    res["rt_mass"] = dict(two_rhs=rt_mass.two_rhs(), streams=rt_mass.streams())
    res["lanes"] = dict(nd=[c_nd.lanes(), c_nd.lanes(True)], rt=[c_rt.lanes(), c_rt.lanes(True)])
    Mc_nd = linalg.ComplexParOperator(ctx, nd_mass, None, conforming=c_nd)
    Mc_rt = linalg.ComplexParOperator(ctx, rt_mass, None, conforming=c_rt)

    # the same estimate on the unrefined mesh, no constraints
    c_mat, c_sq, c_isq = mh.estimator_materials([np.eye(3)])
    geom0 = ceed.GeomFactorData(m0, p + 1)
    flux0 = ceed.mixedmass_operator(geom0, rt0, nd0, c_mat.pack())
    mass0 = ceed.ndmass_operator(geom0, nd0, po.CoeffCtx().pack())
    M0 = linalg.ParOperator(ctx, mass0, np.zeros(0, np.int32), linalg.DIAG_ONE)
    cg0 = linalg.cg(ctx, M0, linalg.jacobi(ctx, M0), rel_tol=1e-13, max_it=1000)
    integ0 = ceed.HexElementErrorIntegrator(geom0, rt0, nd0, ceed.QF_HDIVHCURL_ERROR_33, np.concatenate([c_sq.pack(), c_isq.pack()]))
    B0, rhs0, H0, e0v = new(rt0.ndofs), new(nd0.ndofs), new(nd0.ndofs), new(m0.ne)
    Bc = new(rt.n_true)
    its = {}

    def estimate_unrefined():
        flux0.mult(B0, rhs0)
        H0.zero_()
        cg0.mult(rhs0, H0)
        e0v.zero_()
        integ0.apply_add(B0, H0, e0v)
        its["unrefined"] = cg0.stats()["iterations"]

    def estimate_constrained():
        its["constrained"] = est_c.estimate_device(Bc)[2]

    xr, xi, yr, yi = (new(nd.n_true) for _ in range(4))
    lr, li, mr, mi = (new(nd.n_local) for _ in range(4))
    ar, ai, br, bi = (new(rt.n_true) for _ in range(4))
    cr, ci, dr, di = (new(rt.n_local) for _ in range(4))

    def one_pass(c, mass, x0, x1, l0, l1, m0_, m1, y0, y1):
        c.prolongate2(x0, x1, l0, l1)
        mass.mult2(l0, l1, m0_, m1)
        c.restrict2(m0_, m1, y0, y1)

    forms = {
        "prolongate_twice": lambda: (c_nd.prolongate(xr, lr), c_nd.prolongate(xi, li)),
        "prolongate2": lambda: c_nd.prolongate2(xr, xi, lr, li),
        "restrict_twice": lambda: (c_nd.restrict(mr, yr), c_nd.restrict(mi, yi)),
        "restrict2": lambda: c_nd.restrict2(mr, mi, yr, yi),
        "nd_mass_six_launches": lambda: Mc_nd.mult(xr, xi, yr, yi),
        "nd_mass_three_launches": lambda: one_pass(c_nd, nd_mass, xr, xi, lr, li, mr, mi, yr, yi),
        "rt_mass_six_launches": lambda: Mc_rt.mult(ar, ai, br, bi),
        "rt_mass_three_launches": lambda: one_pass(c_rt, rt_mass, ar, ai, cr, ci, dr, di, br, bi),
    }
    whole = {"estimate_constrained": estimate_constrained, "estimate_unrefined": estimate_unrefined}
    for f in forms.values():
        for _ in range(10):
            f()
    for f in whole.values():
        f()
    times = {k: [] for k in list(forms) + list(whole)}
    with torch.cuda.stream(ctx.torch_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):                                                # the forms alternate: five rounds each
            for k, f in list(forms.items()) + list(whole.items()):
                reps = args.reps if k in forms else 1
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps * 1e3)
    res["us"] = {k: dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()}
    res["projector_iterations"] = its
    res["estimate_ns_per_element"] = dict(constrained=round(res["us"]["estimate_constrained"]["median"] * 1e3 / mesh.ne, 1),
                                          unrefined=round(res["us"]["estimate_unrefined"]["median"] * 1e3 / m0.ne, 1))
    print(res, flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
