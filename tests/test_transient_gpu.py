"""palace::TimeOperator on the device (palace_amd/csrc/timeoperator.hip behind linalg.TimeOperator / pa_time_op_*): its
element-wise kernels alone on tiny assembled operators, one step against the reference's literal sequence
(palace_amd.fem.transient.reference_steps) on the O-grid cylinder, and the physics anchors of tests/test_transient_host.py."""
import numpy as np
import pytest

from palace_amd.fem import transient as tr

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_ctx = []


def _context():
    from palace_amd import linalg

    if not _ctx:
        _ctx.append(linalg.Context())
    return _ctx[0]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


# ---- 4. the kernels alone ----------------------------------------------------------------------------------------------

SIZES = [(1, 1), (63, 5), (64, 64), (65, 127), (4099, 1025)]


@pytest.mark.parametrize("rho_inf", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("nE,nB", SIZES)
def test_kernels_on_diagonal_operators(nE, nB, rho_inf):
    """K, C, M diagonal and Curl with two entries per row, all assembled (CSR), Jacobi as the solver of the diagonal systems:
    the solves are exact, so one step (the first of an integration: du/dt = f(u) included) is the kernels' arithmetic.  All data
    positive and the source term negative, so no intermediate sum cancels and every entry of the new state and of the new
    derivative is within 4 eps sum |terms| of its closing sum of at most three products.  Odd nE puts the E block (and k2) at an
    odd offset; the guards around both allocations keep their bits."""
    import scipy.sparse as sp
    import torch

    from palace_amd import ceed, linalg

    ctx = _context()
    rng = np.random.default_rng(1000 * nE + nB)
    kd, cd, md = rng.uniform(0.5, 2.0, nE), rng.uniform(0.1, 0.5, nE), rng.uniform(1.0, 3.0, nE)
    cols = np.stack([rng.integers(0, nE, nB), rng.integers(0, nE, nB)], axis=1)
    if nE > 1:
        cols[:, 1] = (cols[:, 0] + 1 + rng.integers(0, nE - 1, nB)) % nE  # two different columns per row
    else:
        cols = cols[:, :1]
    vals = rng.uniform(0.2, 1.0, cols.shape)
    curl = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, cols.size + 1, cols.shape[1])), shape=(nB, nE))
    dt = 2.0 ** -5
    a = linalg.time_op_stage_factor(rho_inf, dt)
    am, af, gm = tr.generalized_alpha(rho_inf)
    assert a == af * gm / am * dt
    ad = md + a * cd + a * a * kd
    none = np.zeros(0, np.int32)
    mats = [ceed.DeviceCsr.from_scipy(sp.diags(d).tocsr(), symmetric=True) for d in (kd, cd, md, ad)]
    K, C, M, A = [linalg.AssembledParOperator(ctx, m, none, linalg.DIAG_ZERO) for m in mats]
    dcurl = ceed.DeviceCsr.from_scipy(curl)
    curl_op = linalg.CsrInterp(ctx, dcurl)
    negJ = rng.uniform(0.5, 1.0, nE)
    pulse = linalg.pulse("sinusoidal", omega=3.0, t0=-0.8)  # g' < 0 on [0, dt]
    T = linalg.TimeOperator(ctx, K, C, curl_op, linalg.jacobi(ctx, M), linalg.jacobi(ctx, A), _dev(negJ), pulse, rho_inf, dt)
    u1, u2, u3 = rng.uniform(0.5, 1.5, nE), rng.uniform(0.5, 1.5, nE), rng.uniform(0.5, 1.5, nB)
    T.set_state(_dev(u1), _dev(u2), _dev(u3), t=0.0)
    g = T.guard
    assert g == 64
    guards0 = [_host(v(with_guards=True)) for v in (T.state, T.state_dot)]
    assert np.array_equal(_host(T.state()), np.concatenate([u1, u2, u3]))
    T.step()
    assert T.t == dt

    # the same step in numpy, with the magnitudes of the closing sums
    dg0, dg1 = pulse.eval(0.0)[1], pulse.eval(af * dt)[1]
    assert dg0 < 0.0 and dg1 < 0.0
    d1 = (1.0 / md) * (-(kd * u2 + cd * u1) + dg0 * negJ)
    d2, d3 = u1.copy(), -(curl @ u2)
    cp = af * (1.0 - gm / am) * dt
    y1, y2 = u1 + cp * d1, u2 + cp * d2
    k1 = (1.0 / ad) * (-(kd * (y2 + a * y1) + cd * y1) + dg1 * negJ)
    k2 = y1 + a * k1
    k3 = -(curl @ (y2 + a * k2))
    a1, a2, c1, c2 = (1.0 - gm / am) * dt, gm / am * dt, 1.0 - 1.0 / am, 1.0 / am
    u = np.concatenate([u1, u2, u3])
    du = np.concatenate([d1, d2, d3])
    k = np.concatenate([k1, k2, k3])
    want_u, mag_u = u + a1 * du + a2 * k, np.abs(u) + np.abs(a1 * du) + np.abs(a2 * k)
    want_du, mag_du = c1 * du + c2 * k, np.abs(c1 * du) + np.abs(c2 * k)
    got_u, got_du = _host(T.state()), _host(T.state_dot())
    worst = max((np.abs(got_u - want_u) / mag_u).max(), (np.abs(got_du - want_du) / mag_du).max()) / EPS
    print(f"nE {nE} nB {nB} rho {rho_inf}: worst deviation {worst:.2f} eps sum|terms|")
    assert np.all(np.abs(got_u - want_u) <= 4.0 * EPS * mag_u)
    assert np.all(np.abs(got_du - want_du) <= 4.0 * EPS * mag_du)

    st = T.stats()
    # the first step: du/dt = f(u) (three launches) + the step itself (four; five with the stage predictor)
    assert st["predictor_launches"] == (0 if rho_inf == 1.0 else 1)
    assert st["ew_launches"] == 3 + 4 + st["predictor_launches"]
    assert (st["steps"], st["k_applies"], st["c_applies"], st["curl_applies"], st["a_solves"], st["m_solves"]) == (1, 2, 2, 2, 1, 1)
    T.step()
    st2 = T.stats()
    assert st2["ew_launches"] - st["ew_launches"] == (4 if rho_inf == 1.0 else 5)
    assert (st2["k_applies"], st2["c_applies"], st2["curl_applies"], st2["a_solves"], st2["m_solves"]) == (3, 3, 3, 2, 1)
    n = 2 * nE + nB
    for before, view in zip(guards0, (T.state, T.state_dot)):
        after = _host(view(with_guards=True))
        assert after.size == n + 2 * g
        assert before[:g].tobytes() == after[:g].tobytes() and before[-g:].tobytes() == after[-g:].tobytes()
        assert np.all(np.isfinite(after[g:-g]))
    assert T.guards_intact()  # (all six allocations: k with its odd-offset k2 stores, the stage and work vectors too)
    del T
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", [0.1, 0.05])
@pytest.mark.parametrize("rho_inf", [0.1, 0.3, 0.7])
def test_stage_factor_is_one_expression(rho_inf, dt):
    """The stepper asks for exactly the factor pa_time_op_stage_factor returns, for values of rho_inf and dt at which
    alpha_f (gamma / alpha_m) dt and ((alpha_f gamma) / alpha_m) dt round differently (rho_inf = 0.1 with dt = 0.1 or 0.05):
    the C ABI's solver of A(a) is accepted, and two steps on diagonal operators follow the CPU restatement."""
    import scipy.sparse as sp

    from palace_amd import ceed, linalg

    ctx = _context()
    nE, nB = 65, 31
    rng = np.random.default_rng(17)
    kd, cd, md = rng.uniform(0.5, 2.0, nE), rng.uniform(0.1, 0.5, nE), rng.uniform(1.0, 3.0, nE)
    curl = sp.random(nB, nE, density=0.1, random_state=3, format="csr") + sp.csr_matrix((np.ones(nB), (np.arange(nB), np.arange(nB))),
                                                                                        shape=(nB, nE))
    a = linalg.time_op_stage_factor(rho_inf, dt)
    assert a == tr.stage_factor(rho_inf, dt)
    none = np.zeros(0, np.int32)
    mats = [ceed.DeviceCsr.from_scipy(sp.diags(d).tocsr(), symmetric=True) for d in (kd, cd, md, md + a * cd + a * a * kd)]
    K, C, M, A = [linalg.AssembledParOperator(ctx, m, none, linalg.DIAG_ZERO) for m in mats]
    dcurl = ceed.DeviceCsr.from_scipy(curl)
    T = linalg.TimeOperator(ctx, K, C, linalg.CsrInterp(ctx, dcurl), linalg.jacobi(ctx, M), linalg.jacobi(ctx, A), None, None, rho_inf, dt)
    u0 = [rng.uniform(-1, 1, nE), rng.uniform(-1, 1, nE), rng.uniform(-1, 1, nB)]
    T.set_state(*[_dev(b) for b in u0])
    T.step()
    T.step()
    ref = tr.reference_steps(sp.diags(kd), sp.diags(cd), sp.diags(md), curl, None, None, rho_inf, dt, 2, u0=u0)
    dev = np.abs(_host(T.state()) - ref[2]).max() / np.abs(ref[2]).max()
    print(f"rho {rho_inf} dt {dt}: {dev:.2e}")
    assert dev <= 64 * EPS  # (exact solves; a few roundings per entry and step, reordered by the merged applies)
    assert T.stats()["predictor_launches"] == 2 and T.guards_intact()


# ---- 5. one step against the literal sequence ----------------------------------------------------------------------------

# device against reference_steps, relative to each block's peak over the run.  Measured on an MI355X (20 steps, CG to 1e-12):
# at most 1.7e-12 (dE/dt at order 3; 1.0e-12 / 1.6e-12 at orders 1 / 2, 6.6e-13 without damping).  Ten times that, rounded up
# to a power of ten -- well inside the 1e-6 the project asks of solver outputs against the oracle.
GATE = 1e-10


# the coaxial run (test 7) against the CPU restatement: there the device solves to the configuration's 1e-8, not to 1e-12, so the
# deviation is that of the accepted residuals.  Measured on an MI355X relative to each column's peak: at most 1.2e-9 (I[1]; V[1]
# 5.3e-10, V[2] 7.5e-10, I[2] 1.1e-9, E_elec 3.7e-10, E_mag 6.0e-10, the incident columns 0); the gate by the same rule
COAXIAL_GATE = 1e-7


def _ogrid_model(p, damped):
    from palace_amd.fem.mesh import ogrid_cylinder

    mesh = ogrid_cylinder(2, 3)
    mesh.attr[:] = 1 + (np.arange(mesh.ne) % 2)
    rng = np.random.default_rng(7)
    A = rng.uniform(-1, 1, (3, 3))
    mats = dict(attr_mat=[0, 1], eps=[A @ A.T + 2.0 * np.eye(3), 0.7], mu_inv=[1.3, 0.9], sigma=None)
    bfaces = np.nonzero(mesh.boundary_face_mask)[0]
    port = np.zeros(mesh.nfaces, dtype=bool)
    port[bfaces[::3]] = True  # every third boundary face carries the surface term, the others are PEC
    pec = mesh.boundary_face_mask & ~port
    if not damped:
        return tr.HexTransientModel(mesh, p, mats, pec=mesh.boundary_face_mask)
    return tr.HexTransientModel(mesh, p, mats, surfaces=[(port, 0.37)], pec=pec)


def _solvers(ctx, model, dev, a, rel_tol):
    from palace_amd import linalg

    A = model.system(a)
    a_solver = linalg.cg(ctx, A, linalg.jacobi(ctx, A), rel_tol=rel_tol, max_it=2000)
    m_solver = linalg.cg(ctx, dev["M"], linalg.jacobi(ctx, dev["M"]), rel_tol=rel_tol, max_it=2000)
    return A, a_solver, m_solver


@pytest.mark.parametrize("p,damped", [(1, True), (2, True), (3, True), (1, False)])
def test_steps_against_the_literal_sequence(p, damped):
    """20 steps on ogrid_cylinder(2, 3): two attributes, anisotropic eps, a surface mass on part of the boundary and PEC on
    the rest, a source, a random state with zero PEC rows; CG to 1e-12.  Against reference_steps (unmerged applies, sparse LU)
    per block relative to its peak; PEC rows of E and dE/dt exactly zero after every step; one apply of K, C and Curl and one
    solve per step (no C apply without a damping matrix)."""
    import torch

    from palace_amd import linalg

    ctx = _context()
    model = _ogrid_model(p, damped)
    dev = model.device(ctx)
    cpu = model.cpu()
    nE, nB, ess = model.nE, model.nB, model.ess
    assert ess.size and (damped == (cpu["C"] is not None)) and (damped == (dev["C"] is not None))
    rho_inf, dt, n = 1.0, 0.1, 20
    a = linalg.time_op_stage_factor(rho_inf, dt)
    A, a_solver, m_solver = _solvers(ctx, model, dev, a, 1e-12)
    rng = np.random.default_rng(11 + p)
    u0 = [rng.uniform(-1, 1, nE), rng.uniform(-1, 1, nE), rng.uniform(-1, 1, nB)]
    negJ = rng.uniform(-1, 1, nE)
    for v in (u0[0], u0[1], negJ):
        v[ess] = 0.0
    par = dict(omega=4.0, tau=0.6, t0=tr.pulse_delay("mod_gaussian", 0.6) - 2.0)
    ref = tr.reference_steps(cpu["K"], cpu["C"], cpu["M"], cpu["Curl"], negJ, lambda t: tr.pulse_derivative("mod_gaussian", t, **par),
                             rho_inf, dt, n, u0=u0)
    T = linalg.TimeOperator(ctx, dev["K"], dev["C"], dev["Curl"], m_solver, a_solver, _dev(negJ),
                            linalg.pulse("mod_gaussian", **par), rho_inf, dt)
    T.set_state(*[_dev(b) for b in u0])
    ess_d = torch.from_numpy(ess.astype(np.int64)).cuda()
    got = [_host(T.state())]
    for _ in range(n):
        T.step()
        assert bool((T.E[ess_d] == 0.0).all()) and bool((T.Edot[ess_d] == 0.0).all())
        got.append(_host(T.state()))
    got = np.array(got)
    blocks = dict(Edot=slice(0, nE), E=slice(nE, 2 * nE), B=slice(2 * nE, 2 * nE + nB))
    dev_rel = {name: np.abs(got[:, s] - ref[:, s]).max() / np.abs(ref[:, s]).max() for name, s in blocks.items()}
    print(f"p {p} damped {damped}: " + ", ".join(f"{k} {v:.2e}" for k, v in dev_rel.items()))
    st = T.stats()
    assert st["steps"] == n and st["a_solves"] == n and st["m_solves"] == 1
    assert st["k_applies"] == n + 1 and st["curl_applies"] == n + 1  # (+ 1: du/dt = f(u) before the first step)
    assert st["c_applies"] == (n + 1 if damped else 0)
    assert st["ew_launches"] == 3 + 4 * n and st["predictor_launches"] == 0
    assert st["a_iterations"] > 0 and st["m_iterations"] > 0
    for name, v in dev_rel.items():
        assert v <= GATE, (name, v)


# ---- 6. physics on the device ---------------------------------------------------------------------------------------------

def _energy(dev, T, tmp):
    """1/2 (Edot^T M Edot + E^T K E) with the device operators."""
    Ed, E = T.Edot, T.E
    dev["M"].mult(Ed, tmp[0])
    dev["K"].mult(E, tmp[1])
    return 0.5 * float(Ed @ tmp[0] + E @ tmp[1])


def _cylinder_run(cylinder_mesh, rho_inf, n):
    import torch

    from palace_amd import linalg

    ctx = _context()
    mesh = cylinder_mesh
    model = tr.HexTransientModel(mesh, 2, dict(attr_mat=[0] * int(mesh.attr.max()), eps=[2.08], mu_inv=[1.0], sigma=None),
                                 pec=mesh.boundary_face_mask)
    dev = model.device(ctx)
    dt = 0.05
    tol = 1e-12
    A, a_solver, m_solver = _solvers(ctx, model, dev, linalg.time_op_stage_factor(rho_inf, dt), tol)
    T = linalg.TimeOperator(ctx, dev["K"], None, dev["Curl"], m_solver, a_solver, None, None, rho_inf, dt)
    rng = np.random.default_rng(5)
    u0 = [rng.uniform(-1, 1, model.nE), rng.uniform(-1, 1, model.nE), rng.uniform(-1, 1, model.nB)]
    u0[0][model.ess] = 0.0
    u0[1][model.ess] = 0.0
    T.set_state(*[_dev(b) for b in u0])
    tmp = [torch.empty(model.nE, dtype=torch.float64, device="cuda") for _ in range(2)]
    mid, cur = torch.empty(model.nE, dtype=torch.float64, device="cuda"), torch.empty(model.nB, dtype=torch.float64, device="cuda")
    B0 = T.B.clone()
    acc = torch.zeros_like(B0)
    en, far = [_energy(dev, T, tmp)], 0.0
    for _ in range(n):
        E_old = T.E.clone()
        T.step()
        torch.add(E_old, T.E, out=mid)
        mid *= 0.5
        dev["Curl"].mult(mid, cur)
        acc += cur
        far = max(far, float((T.B - (B0 - dt * acc)).abs().max() / T.B.abs().max()))
        en.append(_energy(dev, T, tmp))
    assert T.stats()["c_applies"] == 0
    return np.array(en), far, tol


def test_energy_and_faraday_on_the_device(cylinder_mesh):
    """C = 0, no source, rho_inf = 1, 100 steps on the 80-element cylinder at order 2, CG to 1e-12: the energy drifts by at
    most 100 times the solver tolerance (each step's error is bounded by the residual it accepts; 100 steps), and the Faraday
    sum identity holds to the same bound."""
    en, far, tol = _cylinder_run(cylinder_mesh, 1.0, 100)
    drift = np.abs(en - en[0]).max() / en[0]
    print(f"energy drift {drift:.2e}, Faraday sum {far:.2e}")
    assert drift <= 100.0 * tol
    assert far <= 100.0 * tol


def test_rho_zero_does_not_gain_energy_on_the_device(cylinder_mesh):
    """rho_inf = 0: the energy of the stepper's own sequence never grows (beyond the solver tolerance)."""
    en, _, tol = _cylinder_run(cylinder_mesh, 0.0, 50)
    assert np.all(np.diff(en[1:]) <= 100.0 * tol * en[1])


# ---- 7. the coaxial run on the device ---------------------------------------------------------------------------------------

def test_coaxial_matched_on_the_device():
    """coaxial_matched.json on the device: order 3, 200 steps, PCG to 1e-8 with the p-multigrid [1, 2, 3].  The same columns under
    the same rule as tests/test_transient_host.py against the recorded outputs of the reference; and against the CPU restatement's
    series (direct solves), relative to each column's peak: the device solves to 1e-8 per step where the restatement solves
    exactly, so the series may differ by the accepted residuals of 200 steps."""
    from palace_amd import linalg
    from tests import transient_util as tu

    system = tr.TransientReferenceSystem(_context(), tu.coaxial_mesh())
    T = system.build_device()
    assert abs(linalg.time_op_stage_factor(system.rho_inf, system.dt) - 0.5 * system.dt) <= 1e-16
    series = system.run_device()
    st = T.stats()
    n = system.nsteps
    print(f"A: {st['a_iterations']} iterations in {st['a_solves']} solves; M: {st['m_iterations']} in {st['m_solves']}")
    assert (st["steps"], st["a_solves"], st["k_applies"], st["c_applies"], st["curl_applies"]) == (n, n, n + 1, n + 1, n + 1)
    assert st["ew_launches"] == 3 + 4 * n and st["predictor_launches"] == 0
    tu.check_against_golden(series, "device")
    _, ref = tu.coaxial_reference_run()
    for k in tu.COLUMNS:
        dev = np.abs(series[k] - ref[k]).max() / np.abs(ref[k]).max()
        print(f"device against reference_steps {k}: {dev:.2e}")
        assert dev <= COAXIAL_GATE, (k, dev)
