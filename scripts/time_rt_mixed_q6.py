"""Order-5 flux estimators on the six-point kernels (pa_rt_hex_q6.hip, pa_mixed_hex_q6.hip) on one O-grid cylinder
(cylinder_for_dofs(DOFS, 5), the mesh of scripts/time_hex_q6.py), in one process: the Raviart-Thomas mass apply with packed and
with matrix-free D, the mixed mass H(curl) -> H(div), the element error integrator and a fixed number of PCG + Jacobi
iterations on the RT mass, each at (5, 6) and beside it the (4, 5) kernel of the same family on the SAME mesh.  Every pair is
timed PAIRS times, (5, 6) and (4, 5) alternately, so that the run-to-run spread is visible.  Reported next to each other: the
bytes the algorithm needs (pa_op_algorithmic_bytes; for the error integrator the same count from the shapes) over time for
both kernels and their ratio (lane use alone predicts 36 / 50 = 0.72: 36 of 64 lanes busy against 50 of 64).  There is no
earlier order-5 number: nothing to beat, no gate.
Writes profiles/r15_rt_mixed_q6.json (OUT overrides) and prints it.
  python scripts/time_rt_mixed_q6.py            (PAIRS=5 REPS=20 DOFS=4.0e6 ITS=50)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import cylinder_for_dofs  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", "5"))
REPS = int(os.environ.get("REPS", "20"))
ITS = int(os.environ.get("ITS", "50"))
COPY_TBPS = 6.29
PAIR_LIST = ((5, 6), (4, 5))


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


def summary(ms):
    return {"ms": ms, "ms_median": float(np.median(ms)), "spread": (max(ms) - min(ms)) / float(np.median(ms))}


def alternate(ctx, fns, warm, reps, pairs=None):
    """fns: {key: callable}; every round times each once, in turn."""
    ms = {k: [] for k in fns}
    for _ in range(PAIRS if pairs is None else pairs):
        for k, fn in fns.items():
            ms[k].append(timed(ctx, fn, warm, reps))
    return {k: summary(v) for k, v in ms.items()}


def report(out, name, res, nbytes, kernels):
    """res: alternate() of the keys "5_6" and "4_5"; nbytes: the algorithm's bytes of each."""
    for k in res:
        res[k]["kernel"] = kernels[k]
        res[k]["algorithmic_bytes"] = nbytes[k]
        res[k]["algorithmic_TBps"] = nbytes[k] / (res[k]["ms_median"] * 1e-3) / 1e12
        res[k]["fraction_of_copy_rate"] = res[k]["algorithmic_TBps"] / COPY_TBPS
        res[k]["ns_per_element"] = res[k]["ms_median"] * 1e6 / mesh.ne
    res["bytes_per_time_ratio_5_6_over_4_5"] = res["5_6"]["algorithmic_TBps"] / res["4_5"]["algorithmic_TBps"]
    res["lane_use_prediction"] = 36.0 / 50.0
    out[name] = res


ctx = linalg.Context()
mesh = cylinder_for_dofs(float(os.environ.get("DOFS", "4.0e6")), 5)
nmat = int(mesh.attr.max())
eps = ceed.coefficient_context(3, attr_mat=[0] * nmat, mat_coeff=[np.array([[2.0, 0.3, 0.0], [0.3, 1.5, 0.1], [0.0, 0.1, 1.2]])])
ident = ceed.coefficient_context(3)
gen = torch.Generator(device="cuda").manual_seed(15)
key = {(5, 6): "5_6", (4, 5): "4_5"}
nd, rt, geom = {}, {}, {}
for p, q in PAIR_LIST:
    nd[p], rt[p], geom[p] = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p), ceed.GeomFactorData(mesh, q)


def rand(n):
    return torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)


out = {"workload": f"order-5 flux estimator pieces on {mesh.ne} hexahedra, beside the (4, 5) kernels on the same mesh",
       "elements": int(mesh.ne), "pairs": PAIRS, "reps": REPS, "measured": True,
       "dofs": {key[p, q]: {"nd": nd[p].ndofs, "rt": rt[p].ndofs} for p, q in PAIR_LIST}}

# ---- RT mass apply, packed and matrix-free D
for name, env in (("rt_mass_packed", None), ("rt_mass_matrix_free", "0")):
    if env is not None:
        os.environ["PALACE_AMD_QDATA"] = env  # read at operator creation
    ops = {key[p, q]: ceed.rtmass_operator(geom[p], rt[p], eps) for p, q in PAIR_LIST}
    os.environ.pop("PALACE_AMD_QDATA", None)
    xs = {key[p, q]: rand(rt[p].ndofs) for p, q in PAIR_LIST}
    ys = {k: torch.empty_like(v) for k, v in xs.items()}
    res = alternate(ctx, {k: (lambda k=k: ops[k].mult(xs[k], ys[k])) for k in ops}, 3, REPS)
    report(out, name, res, {k: ops[k].algorithmic_bytes() for k in ops},
           {"5_6": "rt_hex_q6_kernel, one element per wave", "4_5": "rt_hex_apply_kernel, two elements per wave"})
    if env is None:
        rt_ops = ops

# ---- mixed mass H(curl) -> H(div)
ops = {key[p, q]: ceed.mixedmass_operator(geom[p], nd[p], rt[p], eps) for p, q in PAIR_LIST}
xs = {key[p, q]: rand(nd[p].ndofs) for p, q in PAIR_LIST}
ys = {key[p, q]: torch.empty(rt[p].ndofs, dtype=torch.float64, device="cuda") for p, q in PAIR_LIST}
res = alternate(ctx, {k: (lambda k=k: ops[k].mult(xs[k], ys[k])) for k in ops}, 3, REPS)
report(out, "mixed_mass_hcurl_to_hdiv", res, {k: ops[k].algorithmic_bytes() for k in ops},
       {"5_6": "mixed_hex_q6_apply_kernel", "4_5": "mixed_hex_apply_kernel"})

# ---- element error integrator (E in H(curl), D in H(div))
integ = {key[p, q]: ceed.HexElementErrorIntegrator(geom[p], nd[p], rt[p], ceed.QF_HCURLHDIV_ERROR_33, np.concatenate([eps, ident]))
         for p, q in PAIR_LIST}
u1 = {key[p, q]: rand(nd[p].ndofs) for p, q in PAIR_LIST}
u2 = {key[p, q]: rand(rt[p].ndofs) for p, q in PAIR_LIST}
est = {k: torch.zeros(mesh.ne, dtype=torch.float64, device="cuda") for k in integ}
res = alternate(ctx, {k: (lambda k=k: integ[k].apply_add(u1[k], u2[k], est[k])) for k in integ}, 3, REPS)
# what the form reads and writes: 11 geometry rows per point, index (4 B) and slot (2 B) per entry of both spaces, both inputs,
# the estimate read and written
nbytes = {key[p, q]: float(mesh.ne * (q**3 * 11 * 8 + (nd[p].P + rt[p].P) * 6) + 8 * (nd[p].ndofs + rt[p].ndofs) + 16 * mesh.ne)
          for p, q in PAIR_LIST}
report(out, "element_error", res, nbytes, {"5_6": "mixed_hex_q6_error_kernel", "4_5": "mixed_hex_error_kernel"})

# ---- PCG + Jacobi on the RT mass: a fixed number of iterations
solve = {}
stats = {}
for p, q in PAIR_LIST:
    k = key[p, q]
    M = linalg.ParOperator(ctx, rt_ops[k], np.zeros(0, np.int32), linalg.DIAG_ONE)
    K = linalg.cg(ctx, M, linalg.jacobi(ctx, M), rel_tol=0.0, max_it=ITS)
    b, z = torch.empty(rt[p].ndofs, dtype=torch.float64, device="cuda"), torch.empty(rt[p].ndofs, dtype=torch.float64, device="cuda")
    M.mult(torch.ones_like(b), b)

    def run(K=K, b=b, z=z):
        z.zero_()
        K.mult(b, z)

    solve[k], stats[k] = run, K
res = alternate(ctx, solve, 1, 1, pairs=3)
for k in solve:
    st = stats[k].stats()
    res[k].update(iterations=st["iterations"], final_res_over_initial=st["final_res"] / st["initial_res"],
                  iterations_per_s=st["iterations"] / (res[k]["ms_median"] * 1e-3))
res["iterations_per_s_ratio_5_6_over_4_5"] = res["5_6"]["iterations_per_s"] / res["4_5"]["iterations_per_s"]
out["pcg_jacobi_rt_mass"] = res

path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r15_rt_mixed_q6.json"))
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
