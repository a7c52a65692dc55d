"""Both parts of a complex field per pass against two one-part passes, on the bench-size cylinder (cylinder_for_dofs(10e6, 3))
with the rotated sapphire tensor of bench_legs/hex.py, at (p, q1d) = (2, 3), (3, 4) and (4, 5): both directions of the mixed mass
with two right-hand sides (pa_op_mult2), the element error integrator on both parts (pa_error_op_apply_add2) and the
Raviart-Thomas mass on packed D with two right-hand sides.  The one-pass form and PALACE_AMD_TWO_PART=0 alternate in ONE process
(the switch is read at every call), PAIRS times REPS applies each, and every time is listed.  Under the switch the new kernels
are never entered: the comparison is against the kernels of the commit before them.  The one-pass form counts as faster only
where every one of its times is below every one of the other's.  A family and pair without a compiled two-part kernel says so
(one_pass false) and its two columns time the same code.  One JSON line per case and pair.
  python scripts/time_complex_estimator_hex.py            (PAIRS=5 REPS=30 DOFS=10.0e6 PQ=2:3,3:4,4:5)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem import rthex  # noqa: E402
from palace_amd.fem.fespace import NDHexSpace  # noqa: E402
from palace_amd.fem.mesh import cylinder_for_dofs  # noqa: E402

PAIRS = int(os.environ.get("PAIRS", "5"))
REPS = int(os.environ.get("REPS", "30"))
SWITCH = "PALACE_AMD_TWO_PART"


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


def alternate(ctx, fn):
    """(one-pass times, two-pass times): PAIRS pairs of REPS applies, the switch flipped between them."""
    one, two = [], []
    for _ in range(PAIRS):
        os.environ.pop(SWITCH, None)
        one.append(timed(ctx, fn, 5, REPS))
        os.environ[SWITCH] = "0"
        two.append(timed(ctx, fn, 5, REPS))
    os.environ.pop(SWITCH, None)
    return one, two


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


def report(case, p, q1d, nd, sp, one_pass, one, two, diff):
    print(json.dumps({
        "workload": f"{case} p={p} q1d={q1d}, {mesh.ne} hexahedra, ND {nd.ndofs} / RT {sp.ndofs} dofs, rotated sapphire tensor",
        "case": case, "p": p, "q1d": q1d, "elements": int(mesh.ne), "pairs": PAIRS, "reps": REPS, "one_pass": bool(one_pass),
        "one_pass_ms": one, "two_pass_ms": two, "one_pass_ms_median": float(np.median(one)),
        "two_pass_ms_median": float(np.median(two)), "ratio_median": float(np.median(one) / np.median(two)),
        "one_pass_faster_beyond_spread": bool(one_pass and max(one) < min(two)), "max_abs_diff_between_forms": diff}), flush=True)


for p, q1d in pairs:
    nd, sp = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p)
    geom = ceed.GeomFactorData(mesh, q1d)
    gen = torch.Generator(device="cuda").manual_seed(11)
    xs = {id(s): [torch.rand(s.ndofs, dtype=torch.float64, device="cuda", generator=gen) for _ in range(2)] for s in (nd, sp)}

    def two_vectors(op, x, n):
        y = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2)]
        one, two = alternate(ctx, lambda: op.mult2(x[0], x[1], y[0], y[1]))
        ref = [v.clone() for v in y]  # (the last applies ran under the switch)
        op.mult2(x[0], x[1], y[0], y[1])
        return one, two, float(max((a - b).abs().max() for a, b in zip(y, ref)))

    for case, s1, s2 in (("mixed mass ND->RT, two right-hand sides", nd, sp), ("mixed mass RT->ND, two right-hand sides", sp, nd)):
        op = ceed.mixedmass_operator(geom, s1, s2, blob)
        report(case, p, q1d, nd, sp, op.two_rhs(), *two_vectors(op, xs[id(s1)], s2.ndofs))
        del op
    integ = ceed.HexElementErrorIntegrator(geom, nd, sp, ceed.QF_HCURLHDIV_ERROR_33, pair)
    est = torch.zeros(mesh.ne, dtype=torch.float64, device="cuda")
    args = (xs[id(nd)][0], xs[id(sp)][0], xs[id(nd)][1], xs[id(sp)][1])
    one, two = alternate(ctx, lambda: integ.apply_add2(*args, est))
    report("element error ND, RT, both parts", p, q1d, nd, sp, integ.two_parts(), one, two, None)
    del integ
    op = ceed.rtmass_operator(geom, sp, ceed.coefficient_context(3, attr_mat=[0] * nattr, mat_coeff=[np.eye(3)]))
    report("RT mass (packed D), two right-hand sides", p, q1d, nd, sp, op.two_rhs(), *two_vectors(op, xs[id(sp)], sp.ndofs))
    del op, geom
    torch.cuda.empty_cache()
