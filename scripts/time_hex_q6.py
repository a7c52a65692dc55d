"""Order-5 H(curl) hexahedra on the six-point kernel (pa_nd_hex_q6.hip) on one O-grid cylinder (cylinder_for_dofs(DOFS, 5)),
in one process: the K + M ParOperator::Mult at (5, 6), its diagonal, the four coarsened levels (1 ... 4, 6), a fixed number
of PCG + p-multigrid iterations on the levels [1, 2, 3, 5], and beside these the order-4 operator on the SAME mesh on the
one-shot (4, 5) kernel with the streaming form switched off (PALACE_AMD_STREAM5=0) -- the kernel the six-point one was
derived from.  Every apply is timed PAIRS times, (5, 6) and (4, 5) alternately, so that the run-to-run spread is visible.
Reported next to each other: pa_op_algorithmic_bytes / time of both kernels and their ratio (lane use alone predicts 36 / 50
= 0.72: 36 of 64 lanes busy against 50 of 64).  There is no earlier order-5 number: nothing to beat, no gate.
Writes profiles/r14_hex_q6.json (OUT overrides) and prints it.
  python scripts/time_hex_q6.py            (PAIRS=5 REPS=20 DOFS=4.0e6 ITS=20)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import cylinder_for_dofs  # noqa: E402
from palace_amd.fem.partition import levels_for  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", "5"))
REPS = int(os.environ.get("REPS", "20"))
ITS = int(os.environ.get("ITS", "20"))
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


def summary(ms):
    return {"ms": ms, "ms_median": float(np.median(ms)), "spread": (max(ms) - min(ms)) / float(np.median(ms))}


ctx = linalg.Context()
mesh = cylinder_for_dofs(float(os.environ.get("DOFS", "4.0e6")), 5)
mass = ceed.coefficient_context(3, attr_mat=[0] * int(mesh.attr.max()), mat_coeff=[np.array([2.08])])
ident = ceed.coefficient_context(3)
orders = levels_for(5)
assert orders == [1, 2, 3, 5]
spaces = {p: NDHexSpace(mesh, p) for p in (1, 2, 3, 4, 5)}
geom6 = ceed.GeomFactorData(mesh, 6)
fine = ceed.curlcurlmass_operator(geom6, spaces[5], mass, ident)
assert not fine.streams()
os.environ["PALACE_AMD_STREAM5"] = "0"  # read at operator creation
geom5 = ceed.GeomFactorData(mesh, 5)
four = ceed.curlcurlmass_operator(geom5, spaces[4], mass, ident)
del os.environ["PALACE_AMD_STREAM5"]
assert not four.streams()

A5 = linalg.ParOperator(ctx, fine, spaces[5].ess_dofs(), linalg.DIAG_ONE)
A4 = linalg.ParOperator(ctx, four, spaces[4].ess_dofs(), linalg.DIAG_ONE)
gen = torch.Generator(device="cuda").manual_seed(11)
x5 = torch.rand(spaces[5].ndofs, dtype=torch.float64, device="cuda", generator=gen)
x4 = torch.rand(spaces[4].ndofs, dtype=torch.float64, device="cuda", generator=gen)
y5, y4 = torch.empty_like(x5), torch.empty_like(x4)
t5, t4 = [], []
for _ in range(PAIRS):
    t5.append(timed(ctx, lambda: A5.mult(x5, y5), 3, REPS))
    t4.append(timed(ctx, lambda: A4.mult(x4, y4), 3, REPS))

out = {"workload": f"K + M on {mesh.ne} hexahedra (scalar mass, identity curl-curl coefficient: the metric form of D)",
       "elements": int(mesh.ne), "pairs": PAIRS, "reps": REPS, "measured": True,
       "mult_5_6": dict(summary(t5), dofs=spaces[5].ndofs, kernel="nd_hex_q6_kernel, one-shot, one element per wave"),
       "mult_4_5_one_shot": dict(summary(t4), dofs=spaces[4].ndofs, kernel="nd_hex_apply_kernel, streaming form off")}
for key, op in (("mult_5_6", fine), ("mult_4_5_one_shot", four)):
    nbytes = op.algorithmic_bytes()
    out[key]["algorithmic_bytes"] = nbytes
    out[key]["algorithmic_TBps"] = nbytes / (out[key]["ms_median"] * 1e-3) / 1e12
    out[key]["fraction_of_copy_rate"] = out[key]["algorithmic_TBps"] / COPY_TBPS
    out[key]["ns_per_element"] = out[key]["ms_median"] * 1e6 / mesh.ne
out["bytes_per_time_ratio_5_6_over_4_5"] = out["mult_5_6"]["algorithmic_TBps"] / out["mult_4_5_one_shot"]["algorithmic_TBps"]
out["lane_use_prediction"] = 36.0 / 50.0

d5 = torch.empty_like(x5)
out["diagonal_5_6"] = summary([timed(ctx, lambda: A5.assemble_diagonal(d5), 1, 3) for _ in range(min(PAIRS, 3))])

local = {p: fine.coarsen(geom6, spaces[p]) for p in (1, 2, 3, 4)}
out["coarsened"] = {}
for p in (1, 2, 3, 4):
    xc = torch.rand(spaces[p].ndofs, dtype=torch.float64, device="cuda", generator=gen)
    yc = torch.empty_like(xc)
    ms = [timed(ctx, lambda: local[p].mult(xc, yc), 3, REPS) for _ in range(PAIRS)]
    nbytes = local[p].algorithmic_bytes()
    out["coarsened"][f"{p}_6"] = dict(summary(ms), dofs=spaces[p].ndofs, algorithmic_bytes=nbytes,
                                      algorithmic_TBps=nbytes / (float(np.median(ms)) * 1e-3) / 1e12)

# PCG + p-multigrid on [1, 2, 3, 5]: a fixed number of iterations (4th-kind Chebyshev of order 10 = 2 p, Jacobi-PCG coarse solve)
A = [linalg.ParOperator(ctx, local[p], spaces[p].ess_dofs(), linalg.DIAG_ONE) for p in orders[:-1]] + [A5]
P = [linalg.Interp(ctx, spaces[a], spaces[b]) for a, b in zip(orders[:-1], orders[1:])]
cs = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1e-2, max_it=8)
B = linalg.gmg(ctx, A, P, cs, cheby_order=10)
K = linalg.cg(ctx, A[-1], B, rel_tol=0.0, max_it=ITS)
b, z = torch.empty_like(x5), torch.empty_like(x5)
A5.mult(torch.ones_like(x5), b)
b[torch.from_numpy(spaces[5].ess_dofs().astype(np.int64)).cuda()] = 0.0


def solve():
    z.zero_()
    K.mult(b, z)


ms = [timed(ctx, solve, 1, 1) for _ in range(3)]
st = K.stats()
out["pcg_gmg_1_2_3_5"] = dict(summary(ms), iterations=st["iterations"], final_res_over_initial=st["final_res"] / st["initial_res"],
                              iterations_per_s=st["iterations"] / (float(np.median(ms)) * 1e-3))
path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "r14_hex_q6.json"))
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)
