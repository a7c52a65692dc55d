"""A / B of the compact-only form of the streaming H(curl) kernel on the bench mesh: the same operators applied with
PALACE_AMD_STREAM_COMPACT=0 and 1 (read at every launch) in one process, alternating, HIP-event timed (ParOperator curl-curl = the
headline step, K + M on the three p-levels = what the smoothers of the PCG loop apply).  PALACE_AMD_LIB selects the build."""
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from palace_amd import ceed, linalg
from palace_amd.fem.partition import SlabProblem

ctx = linalg.Context()
dofs = float(os.environ.get("DOFS", "10e6"))
rounds = int(os.environ.get("ROUNDS", "3"))
prob = SlabProblem(ctx, 0, 1, 3, dofs, levels=True)
mass = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[np.array([2.08])])
fine = ceed.curlcurlmass_operator(prob.geom, prob.spaces[-1], mass, ceed.coefficient_context(3))
ops = {"K(par)": (prob.curlcurl_par_operator(), prob.spaces[-1].ndofs), "K+M p3": (fine, prob.spaces[-1].ndofs)}
for s in prob.spaces[:-1]:
    ops[f"K+M p{s.p}"] = (fine.coarsen(prob.geom, s), s.ndofs)
os.environ["PALACE_AMD_DSTAGE"] = "metric"  # (the metric form of curl-curl alone is not the default: forced for this operator)
ops["Kmet p3"] = (ceed.curlcurl_operator(prob.geom, prob.spaces[-1], ceed.coefficient_context(3)), prob.spaces[-1].ndofs)
del os.environ["PALACE_AMD_DSTAGE"]
print("library", os.environ.get("PALACE_AMD_LIB", "default"), "stream_compact", fine.stream_compact(), "stream_column", fine.stream_column(),
      "stream_affine", fine.stream_affine(), flush=True)
def tm(op, n, sw, reps=50):
    os.environ["PALACE_AMD_STREAM_COMPACT"] = sw
    x = torch.rand(n, dtype=torch.float64, device="cuda"); y = torch.zeros(n, dtype=torch.float64, device="cuda")
    for _ in range(5): op.mult(x, y)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): op.mult(x, y)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
for name, (op, n) in ops.items():  # untimed pass over every operator: the clocks reach their steady state before the first timed round
    for sw in ("0", "1"):
        tm(op, n, sw, reps=100)
for rnd in range(rounds):
    for name, (op, n) in ops.items():
        row = [tm(op, n, sw) for sw in ("0", "1")]
        print(f"round {rnd} {name:8s} compact off {row[0]:7.1f} us   on {row[1]:7.1f} us   ({100 * (row[1] / row[0] - 1):+.1f} %)", flush=True)
