"""The three-point streaming H(curl) hex kernel (pa_nd_hex_stream3.hip, PALACE_AMD_STREAM3=1) against the one-shot kernel that is
the default at that rule, on the bench cylinder (125 440 elements), in one process.

A. `ParOperator::Mult` (PEC essential rows fused) at order 2 on its own rule and at order 1 on the same rule (the coarsened
   level): curl-curl and mass on packed D, K + M on the metric form and on packed anisotropic D.  The two operators of a form are
   created side by side (switch off / on) and timed alternately, PAIRS times REPS applies each; reported per form: the median
   and the range of the pairs in us, the achieved bytes/s on NE (27 G 8 + P 5) + 16 N with the G actually streamed, and the
   relative l2 difference of y between the two kernels at this size.
B. PCG + p-multigrid: the order-2 problem with levels (1, 2), 50 iterations and to 1e-8, switch off / on; the order-3 bench
   problem with level_rule="fine" against level_rule="own" with the switch on.

    python scripts/time_stream3_hex.py [out.json]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from palace_amd import ceed, linalg  # noqa: E402
from palace_amd.fem.partition import SlabProblem, strong_shape  # noqa: E402

SWITCH = "PALACE_AMD_STREAM3"
PAIRS, REPS = 7, 40
Q1D = 3


def switch(on):
    if on:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)


def aniso_context(nattr):
    A = np.random.default_rng(7).uniform(-1, 1, (3, 3))
    return ceed.coefficient_context(3, attr_mat=[0] * nattr, mat_coeff=[A @ A.T + 2.0 * np.eye(3)])


def time_us(ctx, A, x, y, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ctx.torch_stream):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            A.mult(x, y)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def apply_table(ctx, out):
    shape = strong_shape(10.0e6, 3)  # the bench cylinder
    prob = SlabProblem(ctx, 0, 1, 2, 0.0, levels=True, shape=shape)  # orders (1, 2), three points per direction
    assert prob.q1d == Q1D
    mesh, geom = prob.mesh, prob.geom
    nattr = int(mesh.attr.max())
    mass = ceed.coefficient_context(3, attr_mat=[0] * nattr, mat_coeff=[np.array([2.08])])
    ident = ceed.coefficient_context(3)
    aniso = aniso_context(nattr)
    forms = [("curl-curl, packed D", 6, lambda g, s: ceed.curlcurl_operator(g, s, ident)),
             ("mass, packed D", 6, lambda g, s: ceed.ndmass_operator(g, s, mass)),
             ("K + M, metric form", 7, lambda g, s: ceed.curlcurlmass_operator(g, s, mass, ident)),
             ("K + M, packed anisotropic D", 12, lambda g, s: ceed.curlcurlmass_operator(g, s, mass, aniso))]
    out["elements"] = int(mesh.ne)
    out["apply"] = []
    fine_space = prob.spaces[-1]
    for p, space, ess in ((2, prob.spaces[1], prob.ess[1]), (1, prob.spaces[0], prob.ess[0])):
        n, P = space.ndofs, 3 * p * (p + 1) ** 2
        x = torch.rand(n, dtype=torch.float64, device="cuda")
        for name, G, make in forms:
            ops, keep = [], []
            for on in (False, True):
                switch(on)
                fine = make(geom, fine_space)
                local = fine if p == 2 else fine.coarsen(geom, space)
                keep.append(fine)
                assert local.streams() == on, (name, p, on)
                ops.append(linalg.ParOperator(ctx, local, ess, linalg.DIAG_ONE))
            switch(False)
            ys = [torch.empty_like(x), torch.empty_like(x)]
            for A, y in zip(ops, ys):
                for _ in range(10):
                    A.mult(x, y)
            torch.cuda.synchronize()
            diff = float((ys[0] - ys[1]).norm() / ys[0].norm())
            t = [[], []]
            for _ in range(PAIRS):
                for k in (0, 1):
                    t[k].append(time_us(ctx, ops[k], x, ys[k], REPS))
            nbytes = mesh.ne * (27 * G * 8 + P * 5) + 16 * n
            row = {"order": p, "form": name, "G": G, "dofs": n, "bytes": nbytes, "rel_l2_y_stream_vs_one_shot": diff}
            for k, key in ((0, "one_shot"), (1, "stream3")):
                med = statistics.median(t[k])
                row[key] = {"us_median": med, "us_min": min(t[k]), "us_max": max(t[k]), "TBps_median": nbytes / med / 1e6}
            row["stream3_over_one_shot"] = row["stream3"]["us_median"] / row["one_shot"]["us_median"]
            out["apply"].append(row)
            print(f"p = {p} {name:28s}: one-shot {row['one_shot']['us_median']:7.1f} us [{min(t[0]):.1f}, {max(t[0]):.1f}]"
                  f" {row['one_shot']['TBps_median']:.2f} TB/s | stream3 {row['stream3']['us_median']:7.1f} us [{min(t[1]):.1f}, {max(t[1]):.1f}]"
                  f" {row['stream3']['TBps_median']:.2f} TB/s | ratio {row['stream3_over_one_shot']:.3f} | rel diff of y {diff:.1e}", flush=True)
            del ops, keep, ys
    return prob


def solve(prob, **kw):
    """(it/s over 50 iterations, iterations to 1e-8, seconds to 1e-8)"""
    K, b, x = prob.pcg_gmg_solver(max_it=50, hiptmair=False, coarse="chebyshev", **kw)
    K.mult(b, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K.mult(b, x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    its = K.stats()["iterations"]
    del K
    prob._keep.clear()
    K, b, x = prob.pcg_gmg_solver(max_it=400, rel_tol=1e-8, hiptmair=False, coarse="chebyshev", **kw)
    K.mult(b, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K.mult(b, x)
    torch.cuda.synchronize()
    dt8 = time.perf_counter() - t0
    st = K.stats()
    del K
    prob._keep.clear()
    return {"it_per_s_50": its / dt, "iterations_to_1e-8": st["iterations"], "seconds_to_1e-8": dt8, "converged": bool(st["converged"])}


def main():
    ctx = linalg.Context()
    out = {"what": "three-point streaming H(curl) hex kernel (PALACE_AMD_STREAM3=1) against the one-shot kernel, same process, A / B pairs",
           "pairs": PAIRS, "reps_per_pair": REPS, "bytes_formula": "NE*(27*G*8 + P*5) + 16*N, G = q-data doubles per point actually streamed"}
    prob2 = apply_table(ctx, out)
    out["pcg_order2_levels_1_2"] = {}
    for rnd in (0, 1):
        for on in (False, True):
            switch(on)
            r = solve(prob2)
            out["pcg_order2_levels_1_2"].setdefault("stream3" if on else "one_shot", []).append(r)
            print(f"order 2, levels (1, 2), switch {'on ' if on else 'off'}: {r}", flush=True)
    switch(False)
    del prob2
    prob3 = SlabProblem(ctx, 0, 1, 3, 10.0e6, levels=True, shape=strong_shape(10.0e6, 3))
    out["pcg_order3_bench"] = {}
    for rnd in (0, 1):
        for rule, on in (("fine", False), ("own", True)):
            switch(on)
            r = solve(prob3, level_rule=rule)
            out["pcg_order3_bench"].setdefault(f"level_rule={rule}" + (", stream3" if on else ""), []).append(r)
            print(f"order 3 bench problem, level_rule = {rule}, switch {'on ' if on else 'off'}: {r}", flush=True)
    switch(False)
    path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r13_stream3_hex.json"
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("written", path)


if __name__ == "__main__":
    main()
