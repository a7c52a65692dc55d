"""Order 4 (five points per direction) with anisotropic materials on the bench mesh, ~10M dofs: ComplexParOperator::Mult of
A = (K - w^2 eps M) + i w sigma M with the rotated sapphire tensors of bench_legs/hex.py: complex_leg(aniso=True), and the real
anisotropic K + M ParOperator::Mult alone (packed D, 12 doubles per point).  Prints one JSON line with both times, the capability
queries (pa_op_streams of the real operator, pa_op_complex_fused of the pair), the value of PALACE_AMD_COMPLEX_FUSED the process
ran under (the switch is read once per process: the unfused time is a second run) and a checksum of the complex result, so that
two runs -- two settings of the switch, two builds of the library -- can be compared.
  python scripts/time_complex_aniso_p4.py; PALACE_AMD_COMPLEX_FUSED=0 python scripts/time_complex_aniso_p4.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.partition import SlabProblem  # noqa: E402

REPS = int(os.environ.get("REPS", "50"))


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
prob = SlabProblem(ctx, 0, 1, 4, float(os.environ.get("DOFS", "10.0e6")), levels=False)
nd = prob.spaces[-1]
n = nd.ndofs
c, s_ = np.cos(0.3), np.sin(0.3)
R = np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s_], [0.0, s_, c]])
eps = R @ np.diag([9.3, 9.3, 11.5]) @ R.T
loss = R @ np.diag([9.3 * 3.0e-5, 9.3 * 3.0e-5, 11.5 * 8.6e-5]) @ R.T
eps, loss = 0.5 * (eps + eps.T), 0.5 * (loss + loss.T)  # (exactly symmetric: the packed form is chosen on an exact test)
mass = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[-0.3 * eps])
cond = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[0.3 * loss])
Ar = ceed.curlcurlmass_operator(prob.geom, nd, mass, ceed.coefficient_context(3))
Ai = ceed.ndmass_operator(prob.geom, nd, cond)
lib = ceed._lib.load()
out = {"workload": f"ND p={nd.p}, {prob.mesh.ne} hexahedra, five points per direction, {n} dofs, rotated sapphire tensors",
       "dofs": n, "elements": int(prob.mesh.ne), "fused_env": os.environ.get("PALACE_AMD_COMPLEX_FUSED", "1"),
       "real_streams": int(lib.pa_op_streams(Ar.handle)), "complex_fused": int(lib.pa_op_complex_fused(Ar.handle, Ai.handle))}

# (i) the real anisotropic K + M
A = linalg.ParOperator(ctx, Ar, prob.ess[-1], linalg.DIAG_ONE)
gen = torch.Generator(device="cuda").manual_seed(11)
xr, xi = (torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(2))
yr, yi = torch.empty_like(xr), torch.empty_like(xr)
out["real_aniso_curlcurl_mass_ms"] = timed(ctx, lambda: A.mult(xr, yr), 10, 2 * REPS)
out["real_checksum"] = float(torch.dot(yr, xi))

# (ii) the complex operator
Ac = linalg.ComplexParOperator(ctx, Ar, Ai, prob.ess[-1], linalg.DIAG_ONE)
out["complex_ms"] = timed(ctx, lambda: Ac.mult(xr, xi, yr, yi), 10, REPS)
out["complex_dof_per_s"] = n / (out["complex_ms"] * 1e-3)
out["complex_checksum"] = [float(torch.dot(yr, xi)), float(torch.dot(yi, xr)), float(yr.norm()), float(yi.norm())]
# bytes as DESIGN.md 3.1c counts them for the four-point form: one pass of both operators' packed D (12 + 6 rows of 126 doubles per
# element) and of the index block (48 words + the slot half-words), two passes (real, imaginary part) of x, y and of the E-vector
# entries of the shared dofs (written by the element kernel, read by the gather; P minus the 3 p (p - 1)^2 interior dofs per element)
p_, ne = nd.p, int(prob.mesh.ne)
P = 3 * p_ * (p_ + 1) ** 2
slots = ((P + 31) // 32 + 1) // 2 * 32 * 4
shared = P - 3 * p_ * (p_ - 1) ** 2
nbytes = ne * ((12 + 6) * 126 * 8 + 48 * 4 + slots) + 2 * (16 * n + 16 * ne * shared)
out["complex_bytes"] = nbytes
out["complex_bytes_formula"] = "NE*((12+6)*126*8 + 48*4 + slots) + 2*(16*N + 16*NE*(P - 3p(p-1)^2))"
out["complex_TBps"] = nbytes / (out["complex_ms"] * 1e-3) / 1e12
print(json.dumps(out))
