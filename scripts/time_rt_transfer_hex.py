"""Raviart-Thomas p-prolongation on the bench-size cylinder (cylinder_for_dofs(10e6, 3), the mesh of time_curl_hex.py) and the
flux projector's mass solve with and without the p-multigrid cycle.

Part 1, pairs (1,2), (2,3), (3,4): P and P^T on the sum-factorised tensor form (pa_prolong_rt_hex.hip behind linalg.Interp), on
the dense interpolator with the same element matrix (linalg.DenseInterp) and, for scale, the Nedelec transfer of the same pair
(interp_kernel_s), timed alternately in one process, PAIRS times each, so that the run-to-run spread is visible.  The bytes are
the necessary traffic computed from the shapes: 4 (P_c + P_f) of index per element, 8 per coarse dof and 8 per fine dof (one
side read, the other written); bytes over time is a WHOLE-OPERATOR rate against the 6.29 TB/s copy rate -- the forward kernel
alone for P, kernel plus gather for P^T (whose E-vector traffic is not counted).

Part 2, orders 2, 3, 4: PCG on the unit-coefficient RT mass of order p (rule p + 1) to TOLS, preconditioned by Jacobi and by the
cycle the flux projector configures with use_mg (levels 1 .. p each assembled on the fine rule, 4th-kind Chebyshev order 2, one
pre and one post step, one native AMG cycle with strength threshold 0.8 on the assembled order-1 level): iterations and
milliseconds per solve, alternated.

One JSON line per pair and per order; with OUT=path the lines are also collected into that file as one JSON list.
  python scripts/time_rt_transfer_hex.py            (PAIRS=5 REPS=30 SOLVES=3 DOFS=10.0e6 TOLS=1e-6,1e-12 ORDERS=2,3,4)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.basis1d import gauss_legendre, gauss_lobatto, lagrange_eval  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import cylinder_for_dofs  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", "5"))
REPS = int(os.environ.get("REPS", "30"))
SOLVES = int(os.environ.get("SOLVES", "3"))
TOLS = [float(v) for v in os.environ.get("TOLS", "1e-6,1e-12").split(",")]
ORDERS = [int(v) for v in os.environ.get("ORDERS", "2,3,4").split(",")]
COPY_TBPS = 6.29
results = []


def emit(out):
    results.append(out)
    print(json.dumps(out), flush=True)


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


def element_matrix(pc, pf):
    """[P_f, P_c] in tensor order: component c is Ic along direction c and Io along the other two."""
    Ic = lagrange_eval(gauss_lobatto(pc + 1), gauss_lobatto(pf + 1))[0]
    Io = lagrange_eval(gauss_legendre(pc)[0], gauss_legendre(pf)[0])[0]
    bc, bf = pc * pc * (pc + 1), pf * pf * (pf + 1)
    M = np.zeros((3 * bf, 3 * bc))
    for c in range(3):
        m = [Ic if d == c else Io for d in range(3)]
        M[c * bf:(c + 1) * bf, c * bc:(c + 1) * bc] = np.kron(m[2], np.kron(m[1], m[0]))
    return M


def summarize(out, name, t, nbytes=None):
    out[f"{name}_ms"] = t
    out[f"{name}_ms_median"] = float(np.median(t))
    out[f"{name}_spread"] = (max(t) - min(t)) / float(np.median(t))
    if nbytes is not None:
        out[f"{name}_whole_operator_TBps"] = nbytes / (float(np.median(t)) * 1e-3) / 1e12
        out[f"{name}_fraction_of_copy_rate"] = out[f"{name}_whole_operator_TBps"] / COPY_TBPS


ctx = linalg.Context()
mesh = cylinder_for_dofs(float(os.environ.get("DOFS", "10.0e6")), 3)
rt_spaces, nd_spaces = {}, {}


def rt_space(p):
    if p not in rt_spaces:
        rt_spaces[p] = rthex.RTHexSpace(mesh, p)
    return rt_spaces[p]


def nd_space(p):
    if p not in nd_spaces:
        nd_spaces[p] = NDHexSpace(mesh, p)
    return nd_spaces[p]


# ---- part 1: the transfers
for pf in ORDERS:
    pc = pf - 1
    c, f = rt_space(pc), rt_space(pf)
    nc, nf = nd_space(pc), nd_space(pf)
    ops = {"tensor": linalg.Interp(ctx, c, f), "dense": linalg.DenseInterp(ctx, c.restriction(), f.restriction(), element_matrix(pc, pf)),
           "nedelec": linalg.Interp(ctx, nc, nf)}
    gen = torch.Generator(device="cuda").manual_seed(12)
    xs = {k: (torch.rand((nc if k == "nedelec" else c).ndofs, dtype=torch.float64, device="cuda", generator=gen),
              torch.rand((nf if k == "nedelec" else f).ndofs, dtype=torch.float64, device="cuda", generator=gen)) for k in ops}
    xs["dense"] = xs["tensor"]
    ys = {k: (torch.empty_like(xs[k][1]), torch.empty_like(xs[k][0])) for k in ops}
    ms = {k + d: [] for k in ops for d in ("_P", "_Pt")}
    for _ in range(PAIRS):
        for k, op in ops.items():
            ms[k + "_P"].append(timed(ctx, lambda: op.mult(xs[k][0], ys[k][0]), 5, REPS))
        for k, op in ops.items():
            ms[k + "_Pt"].append(timed(ctx, lambda: op.mult_transpose(xs[k][1], ys[k][1]), 5, REPS))
    nb_rt = int(mesh.ne) * 4 * (c.P + f.P) + 8 * c.ndofs + 8 * f.ndofs
    nb_nd = int(mesh.ne) * 4 * (nc.P + nf.P) + 8 * nc.ndofs + 8 * nf.ndofs
    out = {"workload": f"RT p-prolongation ({pc}, {pf}), {mesh.ne} hexahedra, {c.ndofs} coarse and {f.ndofs} fine RT dofs",
           "kind": "transfer", "pc": pc, "pf": pf, "elements": int(mesh.ne), "rt_dofs": [c.ndofs, f.ndofs],
           "nd_dofs": [nc.ndofs, nf.ndofs], "pairs": PAIRS, "reps": REPS, "necessary_bytes_rt": nb_rt, "necessary_bytes_nd": nb_nd}
    for d in ("P", "Pt"):
        summarize(out, f"tensor_{d}", ms[f"tensor_{d}"], nb_rt)
        summarize(out, f"dense_{d}", ms[f"dense_{d}"], nb_rt)
        summarize(out, f"nedelec_{d}", ms[f"nedelec_{d}"], nb_nd)
        out[f"speedup_over_dense_{d}_median"] = float(np.median(ms[f"dense_{d}"]) / np.median(ms[f"tensor_{d}"]))
        out[f"tensor_{d}_faster_than_dense_beyond_spread"] = bool(max(ms[f"tensor_{d}"]) < min(ms[f"dense_{d}"]))
    out["max_rel_diff_P"] = float((ys["tensor"][0] - ys["dense"][0]).abs().max() / ys["dense"][0].abs().max())
    out["max_rel_diff_Pt"] = float((ys["tensor"][1] - ys["dense"][1]).abs().max() / ys["dense"][1].abs().max())
    emit(out)
    del ops, xs, ys
    torch.cuda.empty_cache()
nd_spaces.clear()

# ---- part 2: the projector's mass solve
blob = ceed.coefficient_context(3)
none = np.zeros(0, dtype=np.int32)
for p in ORDERS:
    geom = ceed.GeomFactorData(mesh, p + 1)
    sp = [rt_space(l) for l in range(1, p + 1)]
    local = [ceed.rtmass_operator(geom, s, blob) for s in sp]
    A = [linalg.ParOperator(ctx, op, none) for op in local]
    P = [linalg.Interp(ctx, sp[l], sp[l + 1]) for l in range(p - 1)]
    coarse = linalg.amg(ctx, local[0].full_assemble_device(), theta=0.8)
    amg_levels = len(linalg.amg_hierarchy(coarse)[0])
    B = linalg.gmg(ctx, A, P, coarse, cheby_order=2)
    J = linalg.jacobi(ctx, A[-1])
    n = sp[-1].ndofs
    gen = torch.Generator(device="cuda").manual_seed(21)
    x0 = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    b = A[-1].mult(x0, torch.empty_like(x0))
    out = {"workload": f"RT mass solve p={p}, {mesh.ne} hexahedra, {n} dofs, levels 1..{p}", "kind": "solve", "p": p, "dofs": n,
           "level_dofs": [s.ndofs for s in sp], "coarse_amg_levels": amg_levels, "solves": SOLVES, "tols": TOLS}
    for tol in TOLS:
        K = {"jacobi": linalg.cg(ctx, A[-1], J, rel_tol=tol, max_it=1000), "mg": linalg.cg(ctx, A[-1], B, rel_tol=tol, max_it=1000)}
        x = {k: torch.zeros_like(x0) for k in K}
        ms = {k: [] for k in K}
        for _ in range(SOLVES):
            for k, s in K.items():
                ms[k].append(timed(ctx, lambda: s.mult(b, x[k]), 1, 2))
        tag = f"tol_{tol:.0e}"
        for k, s in K.items():
            st = s.stats()
            out[f"{tag}_{k}_iterations"] = int(st["iterations"])
            out[f"{tag}_{k}_converged"] = bool(st["converged"])
            out[f"{tag}_{k}_error"] = float((x[k] - x0).norm() / x0.norm())
            summarize(out, f"{tag}_{k}", ms[k])
        out[f"{tag}_mg_over_jacobi_time"] = out[f"{tag}_mg_ms_median"] / out[f"{tag}_jacobi_ms_median"]
        out[f"{tag}_mg_faster_beyond_spread"] = bool(max(ms["mg"]) < min(ms["jacobi"]))
        del K
    emit(out)
    del A, P, B, J, coarse, local, geom
    torch.cuda.empty_cache()

if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
