"""Time one transient step (palace_amd.linalg.TimeOperator, rho_inf = 1) against the same step written with the calls that
existed before it (ParOperator applies, pa_vec_axpby, the same solver) in the reference's literal order
(models/timeoperator.cpp:113-223 under mfem::GeneralizedAlphaSolver::Step), and against the solve alone.

    python scripts/time_transient.py [--dofs 1e7] [--steps 10] [--blocks 3] [--out profiles/r20_transient.json]

The mesh is cylinder_for_dofs(dofs, 3): order 3, PEC on the mantle, a surface mass (a lumped-port style 1 / R_s term) on the two
caps, a modulated Gaussian source.  Both forms advance their own copy of the same state with the same A(a) solver (PCG to 1e-8,
p-multigrid [1, 2, 3]); blocks of `steps` steps alternate between them after a warm-up, every block ends in a device
synchronise, and the per-step wall time is reported per block.  The literal form makes 14 vector passes per step, a few more
than the reference's own sequence (about ten): pa_vec_axpby has two operands, so y = u + 0 du, k2 and k3 each take a copy and an
update.  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dofs", type=float, default=1e7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from palace_amd import lib as _lib
    from palace_amd import linalg
    from palace_amd.fem import transient as tr
    from palace_amd.fem.mesh import cylinder_for_dofs

    assert torch.cuda.is_available(), "time_transient.py measures on the GPU"
    L = linalg._L()
    ctx = linalg.Context()
    p = 3
    mesh = cylinder_for_dofs(args.dofs, p)
    # caps: boundary faces whose four vertices share z
    fz = mesh.vert_coords[mesh.face_verts][:, :, 2]
    cap = mesh.boundary_face_mask & (np.ptp(fz, axis=1) < 1e-9)
    pec = mesh.boundary_face_mask & ~cap
    mats = dict(attr_mat=[0] * int(mesh.attr.max()), eps=[2.08], mu_inv=[1.0], sigma=None)
    model = tr.HexTransientModel(mesh, p, mats, surfaces=[(cap, 0.7)], pec=pec)
    dev = model.device(ctx)
    nE, nB = model.nE, model.nB
    # a step that resolves the elements: dt ~ the element size
    h = float(np.linalg.norm(mesh.vert_coords[mesh.edge_verts[:, 0]] - mesh.vert_coords[mesh.edge_verts[:, 1]], axis=1).mean())
    dt, rho_inf = h, 1.0
    a = linalg.time_op_stage_factor(rho_inf, dt)
    _, A, _, gmg, a_solver = tr.pmg_system_solver(ctx, model, a, 1e-8, 100)
    m_solver = linalg.cg(ctx, dev["M"], linalg.jacobi(ctx, dev["M"]), rel_tol=1e-8, max_it=100)
    rng = np.random.default_rng(3)
    negJ = rng.uniform(-1, 1, nE)
    negJ[model.ess] = 0.0
    negJ_d = torch.from_numpy(negJ).cuda()
    par = dict(omega=2.0 * np.pi / (20 * dt), tau=10 * dt)
    par["t0"] = tr.pulse_delay("mod_gaussian", par["tau"])
    T = linalg.TimeOperator(ctx, dev["K"], dev["C"], dev["Curl"], m_solver, a_solver, negJ_d, linalg.pulse("mod_gaussian", **par),
                            rho_inf, dt)
    T.init(0.0)

    # ---- the literal step on the pre-existing calls (rho_inf = 1: alpha_m = alpha_f = gamma = 1/2) -------------------------
    n = 2 * nE + nB
    new = lambda m: torch.zeros(m, dtype=torch.float64, device="cuda")  # noqa: E731
    u, du, y, k, rhs, tmpB = new(n), new(n), new(n), new(n), new(n), new(nB)
    s1, s2, s3 = slice(0, nE), slice(nE, 2 * nE), slice(2 * nE, n)
    passes = [0]

    def axpby(al, x, be, yv):
        _lib.check(L.pa_vec_axpby(ctx.handle, al, C.c_void_p(x.data_ptr()), be, C.c_void_p(yv.data_ptr()), x.numel()))
        passes[0] += 1

    def form_rhs(v, t):
        dev["K"].mult(v[s2], rhs[s1])
        dev["C"].add_mult(v[s1], rhs[s1], 1.0)
        axpby(float(tr.pulse_derivative("mod_gaussian", t, **par)), negJ_d, -1.0, rhs[s1])
        axpby(1.0, v[s1], 0.0, rhs[s2])
        dev["Curl"].mult(v[s2], rhs[s3])
        axpby(0.0, rhs[s3], -1.0, rhs[s3])

    state = dict(t=0.0, first=True, snap=False)

    def literal_step():
        t = state["t"]
        if state["first"]:
            form_rhs(u, t)
            m_solver.mult(rhs[s1], du[s1])
            axpby(1.0, rhs[s2], 0.0, du[s2])
            axpby(1.0, rhs[s3], 0.0, du[s3])
            state["first"] = False
        axpby(1.0, u, 0.0, y)                      # add(x, dt_fac1 dt, xdot, y) with dt_fac1 = 0
        axpby(0.0, du, 1.0, y)
        form_rhs(y, t + 0.5 * dt)
        dev["K"].add_mult(rhs[s2], rhs[s1], -a)
        if state["snap"]:  # the system of this step and its starting iterate, for the solve timed alone
            state["rhs"], state["x0"], state["snap"] = rhs[s1].clone(), k[s1].clone(), False
        a_solver.mult(rhs[s1], k[s1], initial_guess=True)
        axpby(1.0, rhs[s2], 0.0, k[s2])            # k2 = rhs2 + a k1
        axpby(a, k[s1], 1.0, k[s2])
        axpby(1.0, rhs[s3], 0.0, k[s3])            # k3 = rhs3 - a Curl k2
        dev["Curl"].mult(k[s2], tmpB)
        axpby(-a, tmpB, 1.0, k[s3])
        axpby(a, k, 1.0, y)                        # add(y, dt_fac2 dt, k, y)
        axpby(0.0, y, -1.0, u)                     # x *= 1 - 1 / alpha_f
        axpby(2.0, y, 1.0, u)                      # x += y / alpha_f
        axpby(-1.0, du, 1.0, k)                    # k -= xdot
        axpby(2.0, k, 1.0, du)                     # xdot += k / alpha_m
        state["t"] = t + dt

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    # ---- warm-up, the parity of the two forms, the alternating blocks ------------------------------------------------------
    for _ in range(3):
        T.step()
        literal_step()
    torch.cuda.synchronize()
    dev_rel = float((T.state() - u).abs().max() / u.abs().max())
    p0, state["snap"] = passes[0], True
    literal_step()
    T.step()
    passes_per_step = passes[0] - p0
    rhs_solve, x_solve = state["rhs"], torch.empty_like(state["x0"])
    res = dict(new_ms=[], literal_ms=[], solve_ms=[])
    for _ in range(args.blocks):
        st0 = T.stats()
        res["new_ms"].append(timed(T.step, args.steps))
        st1 = T.stats()
        res["literal_ms"].append(timed(literal_step, args.steps))
        res["solve_ms"].append(timed(lambda: a_solver.mult(rhs_solve, x_solve.copy_(state["x0"]), initial_guess=True), args.steps))
    out = dict(dofs_E=nE, dofs_B=nB, elements=mesh.ne, order=p, dt=dt, stage_factor=a, steps_per_block=args.steps,
               new_step_ms=res["new_ms"], literal_step_ms=res["literal_ms"], solve_alone_ms=res["solve_ms"],
               a_iterations_per_step_last_block=(st1["a_iterations"] - st0["a_iterations"]) / args.steps,
               literal_vector_passes_per_step=passes_per_step, new_elementwise_launches_per_step=4,
               state_deviation_after_warmup=dev_rel, stats=T.stats())
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
