"""Transient solves on hexahedra: the first-order system (dE/dt, E, B) of the reference's time operator
(models/timeoperator.cpp:22-282) and its generalized-alpha stepper, as a CPU restatement (`reference_steps`: the reference's
literal sequence with sparse direct solves) and as the device set-up for palace_amd.linalg.TimeOperator (`HexTransientModel`, `TransientReferenceSystem`).

    M u1' = -(K u2 + C u1) + g'(t) NegJ        K, C: DIAG_ZERO on the PEC rows, M: DIAG_ONE
      u2' = u1
      u3' = -Curl u2

The stepper (Jansen, Whiting, Hulbert 2000; the reference takes rho_inf = 1):
    alpha_m = (3 - rho) / (2 (1 + rho)), alpha_f = 1 / (1 + rho), gamma = 1/2 + alpha_m - alpha_f
    first step:  du = Mult(u) at t0
    y  = u + alpha_f (1 - gamma / alpha_m) dt du
    k  = ImplicitSolve(alpha_f gamma / alpha_m dt, y) at t + alpha_f dt
    u  = u + (1 - gamma / alpha_m) dt du + gamma / alpha_m dt k
    du = (1 - 1 / alpha_m) du + k / alpha_m
"""
from __future__ import annotations

import numpy as np

# ---- excitation pulses (utils/excitations.hpp), value and derivative ------------------------------------------------------

PULSE_KINDS = ("sinusoidal", "gaussian", "diff_gaussian", "mod_gaussian", "ramp", "smooth_step")


def pulse_delay(kind, tau):
    """The delay the reference's driver applies (drivers/transientsolver.cpp:135-138): 4.5 tau for the Gaussian shapes."""
    return 4.5 * tau if kind in ("gaussian", "diff_gaussian", "mod_gaussian") else 0.0


def pulse_value(kind, t, omega=0.0, tau=0.0, t0=0.0):
    ts = t - t0
    if kind == "sinusoidal":
        return np.sin(omega * ts)
    if kind == "gaussian":
        return np.exp(-0.5 * ts * ts / (tau * tau))
    if kind == "diff_gaussian":
        return -ts / (tau * tau) * np.exp(-0.5 * ts * ts / (tau * tau))
    if kind == "mod_gaussian":
        return np.sin(omega * ts) * np.exp(-0.5 * ts * ts / (tau * tau))
    s = np.clip(ts / tau, 0.0, 1.0)
    if kind == "ramp":
        return s
    if kind == "smooth_step":
        return s ** 3 * (6.0 * s * s - 15.0 * s + 10.0)
    raise ValueError(kind)


def pulse_derivative(kind, t, omega=0.0, tau=0.0, t0=0.0):
    ts = t - t0
    if kind == "sinusoidal":
        return omega * np.cos(omega * ts)
    oot2 = 1.0 / (tau * tau)
    g = np.exp(-0.5 * ts * ts * oot2)
    if kind == "gaussian":
        return -ts * oot2 * g
    if kind == "diff_gaussian":
        return -oot2 * (1.0 - ts * ts * oot2) * g
    if kind == "mod_gaussian":
        return (-ts * oot2 * np.sin(omega * ts) + omega * np.cos(omega * ts)) * g
    s = np.clip(ts / tau, 0.0, 1.0)
    inside = (ts > 0.0) & (ts < tau)
    if kind == "ramp":
        return np.where(inside, 1.0 / tau, 0.0)
    if kind == "smooth_step":
        return 30.0 * s * s * (s - 1.0) ** 2 / tau
    raise ValueError(kind)


# ---- the stepper ---------------------------------------------------------------------------------------------------------

def generalized_alpha(rho_inf):
    """(alpha_m, alpha_f, gamma)."""
    alpha_m = 0.5 * (3.0 - rho_inf) / (1.0 + rho_inf)
    alpha_f = 1.0 / (1.0 + rho_inf)
    return alpha_m, alpha_f, 0.5 + alpha_m - alpha_f


def stage_factor(rho_inf, dt):
    """a = alpha_f gamma / alpha_m dt: the factor of A(a) = M + a C + a^2 K (dt / 2 for rho_inf = 1)."""
    alpha_m, alpha_f, gamma = generalized_alpha(rho_inf)
    return alpha_f * gamma / alpha_m * dt


def reference_steps(K, C, M, Curl, negJ, dg, rho_inf, dt, n, u0=None, t0=0.0, observe=None):
    """n steps of the reference's LITERAL sequence (unmerged applies; one sparse LU for A, one for M) on scipy matrices that
    already carry the essential-dof policies (K, C: zero rows and columns; M: unit diagonal).  C, negJ, dg may be None.
    u0 = (Edot, E, B) or None (zero).  Returns the states [n + 1, 2 nE + nB], or -- observe(step, t, u) given -- the list of
    its results, one per state."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    nE, nB = K.shape[0], Curl.shape[0]
    K, M, Curl = sp.csr_matrix(K), sp.csr_matrix(M), sp.csr_matrix(Curl)
    C = None if C is None else sp.csr_matrix(C)
    alpha_m, alpha_f, gamma = generalized_alpha(rho_inf)
    a = alpha_f * gamma / alpha_m * dt
    A = M + a * a * K if C is None else M + a * C + a * a * K
    luA, luM = spla.splu(sp.csc_matrix(A)), spla.splu(sp.csc_matrix(M))
    s1, s2, s3 = slice(0, nE), slice(nE, 2 * nE), slice(2 * nE, 2 * nE + nB)

    def form_rhs(u, t):  # timeoperator.cpp:113-146
        rhs = np.empty_like(u)
        r1 = K @ u[s2]
        if C is not None:
            r1 = r1 + C @ u[s1]
        r1 = -1.0 * r1
        if negJ is not None:
            r1 = r1 + dg(t) * negJ
        rhs[s1], rhs[s2], rhs[s3] = r1, u[s1], -(Curl @ u[s2])
        return rhs

    def mult(u, t):  # :152-180
        rhs = form_rhs(u, t)
        rhs[s1] = luM.solve(rhs[s1])
        return rhs

    def implicit_solve(a_, u, t):  # :182-223
        rhs = form_rhs(u, t)
        k = np.empty_like(u)
        k[s1] = luA.solve(rhs[s1] - a_ * (K @ rhs[s2]))
        k[s2] = rhs[s2] + a_ * k[s1]
        k[s3] = rhs[s3] - a_ * (Curl @ k[s2])
        return k

    u = np.zeros(2 * nE + nB) if u0 is None else np.concatenate([np.asarray(b, dtype=np.float64) for b in u0])
    t = float(t0)
    out = [u.copy() if observe is None else observe(0, t, u)]
    du = None
    for step in range(1, n + 1):
        if du is None:
            du = mult(u, t)
        y = u + (alpha_f * (1.0 - gamma / alpha_m) * dt) * du
        k = implicit_solve(a, y, t + alpha_f * dt)
        u = u + ((1.0 - gamma / alpha_m) * dt) * du + (gamma / alpha_m * dt) * k
        du = (1.0 - 1.0 / alpha_m) * du + (1.0 / alpha_m) * k
        t += dt
        out.append(u.copy() if observe is None else observe(step, t, u))
    return np.array(out) if observe is None else out


# ---- one hexahedral model, assembled for the CPU restatement and for the device --------------------------------------------

def _eliminate(A, ess, diag):
    """Rows and columns `ess` of a scipy matrix zeroed, `diag` on their diagonal (ParOperator's DIAG_ZERO / DIAG_ONE)."""
    import scipy.sparse as sp

    keep = np.ones(A.shape[0])
    keep[ess] = 0.0
    D = sp.diags(keep)
    return (D @ A @ D + sp.diags(diag * (1.0 - keep))).tocsr()


def boundary_face_ids(mesh, quads):
    """Face numbers (mesh.elem_faces numbering) of boundary quadrilaterals given by the node ids of their corners [n, 4]."""
    nv = mesh.nv  # (builds the topology)
    vert_nodes = mesh._topo["vert_nodes"]
    v = np.searchsorted(vert_nodes, np.asarray(quads))
    assert np.array_equal(vert_nodes[v], np.asarray(quads)), "boundary corners are not mesh vertices"
    key = lambda f: (f[:, 0] * nv + f[:, 1]) * nv + f[:, 2]  # noqa: E731  (three smallest vertices, as HexMesh keys its faces)
    table = key(mesh.face_verts.astype(np.int64))
    order = np.argsort(table)
    want = key(np.sort(v, axis=1).astype(np.int64))
    pos = np.searchsorted(table[order], want)
    assert np.array_equal(table[order][pos], want), "a boundary quadrilateral is not a face of the mesh"
    return order[pos]


class HexTransientModel:
    """What a transient run needs on one hexahedral mesh at order p, described once and assembled twice:
      materials  dict(attr_mat=[material of attribute 1, 2, ...], eps=[...], mu_inv=[...], sigma=[...] or None), the entries
                 scalars or symmetric 3 x 3 matrices
      surfaces   [(face mask [nfaces], coefficient)]: surface masses added to C (1 / R_s on a lumped port)
      pec        face mask [nfaces] of the PEC boundary (None: none)
    cpu(): K, C, M with the essential policies, Curl, the unconstrained M_eps and the RT mass M_mu -- scipy matrices from the
    oracle's assemble_sparse and the boundary block's tables.  device(ctx): the same operators as ParOperators / Curl, and
    system(a): A(a) = M + a C + a^2 K as ONE fused volume operator through the sum of coefficient contexts, the surface terms
    beside it."""

    def __init__(self, mesh, p, materials, surfaces=(), pec=None, q1d=None):
        from .fespace import NDHexSpace
        from .rthex import RTHexSpace

        self.mesh, self.p, self.q1d = mesh, p, (p + 1 if q1d is None else q1d)  # (a coarse multigrid level keeps the fine rule)
        self.materials, self.surfaces = materials, list(surfaces)
        self.nd, self.rt = NDHexSpace(mesh, p), RTHexSpace(mesh, p)
        self.nE, self.nB = self.nd.ndofs, self.rt.ndofs
        self.pec = pec
        self.ess = self.nd.ess_dofs(pec) if pec is not None else np.zeros(0, np.int32)
        self._cpu = None

    # -- coefficient contexts ------------------------------------------------------------------------------------------
    def _mats(self, key, scale=1.0):
        return [scale * np.atleast_1d(np.asarray(m, dtype=np.float64)) for m in self.materials[key]]

    def _oracle_ctx(self, key, scale=1.0):
        from oracle import palace_oracle as po

        return po.CoeffCtx(attr_mat=list(self.materials["attr_mat"]), mat_coeff=self._mats(key, scale))

    def _blob(self, key, scale=1.0):
        from .. import ceed

        return ceed.coefficient_context(3, attr_mat=list(self.materials["attr_mat"]), mat_coeff=self._mats(key, scale))

    def has_sigma(self):
        return self.materials.get("sigma") is not None

    def _surface_block(self, mask):
        from .fespace import NDHexBoundaryBlock

        blk = NDHexBoundaryBlock(self.nd, face_mask=mask)
        return blk, blk.tables(self.q1d)

    # -- CPU -----------------------------------------------------------------------------------------------------------
    def cpu(self):
        if self._cpu is not None:
            return self._cpu
        import scipy.sparse as sp

        from oracle import palace_oracle as po
        from . import rthex
        from .basis1d import gauss_legendre

        mesh, p, q1d, nd, rt = self.mesh, self.p, self.q1d, self.nd, self.rt
        _, wts = po.hex_quadrature(q1d)
        G = po.mesh_q2_grad_table(q1d)
        J = np.einsum("dqn,eni->eqid", G, mesh.elem_coords())
        geom = po.build_geom_factor_33(mesh.attr.astype(np.float64), wts, np.transpose(J, (0, 1, 3, 2)).reshape(mesh.ne, -1, 9))
        interp, curl = po.nd_hex_dense_tables(p, q1d, np.arange(nd.P))
        ori = nd.elem_sign_lex < 0

        def volume(qf, key):
            return po.CeedOperatorOracle(nd.ndofs, nd.elem_dof_lex, ori, interp, curl, geom, qf, self._oracle_ctx(key)).assemble_sparse()

        K0, M0 = volume(po.QF_HDIV, "mu_inv"), volume(po.QF_HCURL, "eps")
        C0 = volume(po.QF_HCURL, "sigma") if self.has_sigma() else None
        for mask, coef in self.surfaces:
            blk, (sint, sgrad, sw) = self._surface_block(mask)
            Js = np.einsum("dqn,eni->eqid", sgrad, blk.nodes[blk.elem_nodes])
            og = po.build_geom_factor_32(blk.attr.astype(np.float64), sw, np.transpose(Js, (0, 1, 3, 2)).reshape(blk.ne, -1, 6))
            S = po.CeedOperatorOracle(nd.ndofs, blk.offsets, blk.orients, sint, np.zeros((1, len(sw), blk.P)), og, po.QF_HCURL_32,
                                      po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([float(coef)])])).assemble_sparse()
            C0 = S if C0 is None else C0 + S
        rint, _ = rthex.rt_hex_tables(p, gauss_legendre(q1d)[0])
        Mrt = po.CeedOperatorOracle(rt.ndofs, rt.elem_dof_lex, rt.elem_sign_lex < 0, rint, rint, geom, po.QF_HDIV,
                                    self._oracle_ctx("mu_inv")).assemble_sparse()
        # the discrete curl: every element that holds a flux dof computes the same value; the copies are averaged
        Cm = rthex.hex_curl_matrix(p)
        Pr, Pn = rt.elem_dof_lex.shape[1], nd.P
        val = (rt.elem_sign_lex[:, :, None] * Cm[None] * nd.elem_sign_lex[:, None, :]).astype(np.float64)
        rows = np.repeat(rt.elem_dof_lex[:, :, None], Pn, axis=2)
        cols = np.repeat(nd.elem_dof_lex[:, None, :], Pr, axis=1)
        nz = val != 0.0
        cnt = np.bincount(rt.elem_dof_lex.ravel(), minlength=rt.ndofs).astype(np.float64)
        Curl = sp.coo_matrix((val[nz] / cnt[rows[nz]], (rows[nz], cols[nz])), shape=(rt.ndofs, nd.ndofs)).tocsr()
        ess = self.ess
        self._cpu = dict(K=_eliminate(K0, ess, 0.0), C=None if C0 is None else _eliminate(C0, ess, 0.0), M=_eliminate(M0, ess, 1.0),
                         Curl=Curl, M_eps=M0.tocsr(), M_mu=Mrt.tocsr(), K_free=K0.tocsr())
        return self._cpu

    # -- device --------------------------------------------------------------------------------------------------------
    def device(self, ctx):
        """K, C (None without damping), M as ParOperators with the reference's policies, Curl, and the unconstrained local
        operators M_eps (ND) and M_mu (RT) the energies are measured with."""
        from .. import ceed, linalg

        nd, rt = self.nd, self.rt
        self.prepare(ctx)
        geom, n = self.geom, nd.ndofs
        loc = dict(K=ceed.curlcurl_operator(geom, nd, self._blob("mu_inv")), M=ceed.ndmass_operator(geom, nd, self._blob("eps")),
                   M_mu=ceed.rtmass_operator(geom, rt, self._blob("mu_inv")))
        if self.has_sigma() or self._surf:
            C = ceed.Operator(n, n)
            if self.has_sigma():
                C.add_integrator(geom, nd, ceed.QF_HCURL_33, self._blob("sigma"), ceed.EVAL_INTERP)
            self._add_surfaces(C, 1.0)
            loc["C"] = C.finalize()
        self.local = loc
        d = dict(K=linalg.ParOperator(ctx, loc["K"], self.ess, linalg.DIAG_ZERO),
                 C=linalg.ParOperator(ctx, loc["C"], self.ess, linalg.DIAG_ZERO) if "C" in loc else None,
                 M=linalg.ParOperator(ctx, loc["M"], self.ess, linalg.DIAG_ONE), Curl=linalg.Curl(ctx, nd, rt),
                 M_eps=loc["M"], M_mu=loc["M_mu"])
        self.dev = d
        return d

    def prepare(self, ctx, geom=None):
        """Geometry data and surface blocks on the device: all that system(a) needs (a coarse multigrid level stops here)."""
        from .. import ceed

        self.ctx = ctx
        self.geom = ceed.GeomFactorData(self.mesh, self.q1d) if geom is None else geom
        self._surf = []
        for mask, coef in self.surfaces:
            blk, (sint, sgrad, sw) = self._surface_block(mask)
            sgeom = ceed.DenseGeomFactorData(blk.elem_nodes, blk.nodes, blk.attr, sgrad, sw)
            sblock = ceed.DenseBlock(ceed.FE_HCURL, self.nd.ndofs, blk.offsets, sint, None, orients=blk.orients)
            self._surf.append((sgeom, sblock, float(coef), blk))

    def _add_surfaces(self, op, scale):
        from .. import ceed

        for sgeom, sblock, coef, _ in self._surf:
            blob = ceed.coefficient_context(3, attr_mat=[0], mat_coeff=[np.array([scale * coef])])
            op.add_dense_integrator(sgeom, sblock, ceed.QF_HCURL_32, blob, ceed.EVAL_INTERP)

    def system_local(self, a):
        """The local operator of A(a) = M + a C + a^2 K on the finest space: one fused volume sub-operator (the sum of the
        coefficient contexts, pa_op_add_sub_sum) and the surface masses beside it."""
        from .. import ceed

        nd = self.nd
        terms = [(1.0, ceed.QF_HCURL_33, self._blob("eps")), (a * a, ceed.QF_HDIV_33, self._blob("mu_inv"))]
        if self.has_sigma():
            terms.append((a, ceed.QF_HCURL_33, self._blob("sigma")))
        op = ceed.Operator(nd.ndofs, nd.ndofs).add_integrator_sum(self.geom, nd, terms)
        self._add_surfaces(op, a)
        return op.finalize()

    def system(self, a):
        """ParOperator of A(a) with DIAG_ONE on the PEC rows."""
        from .. import linalg

        loc = self.system_local(a)
        return linalg.ParOperator(self.ctx, loc, self.ess, linalg.DIAG_ONE)


def pmg_system_solver(ctx, fine, a, rel_tol, max_it):
    """PCG on A(a) = M + a C + a^2 K of a HexTransientModel (its device() done) with the p-multigrid V-cycle over the reference's
    order sequence [1, .., p] (fem/multigrid.hpp:44-69): A(a) one fused operator on every level (the coarse levels keep the fine
    quadrature rule and share its geometry data), plain Chebyshev smoothing of order max(2 p, 4) as IoData::CheckConfiguration
    chooses for SPD problems (iodata.cpp:519-564), Jacobi-PCG (8 iterations / 1e-2) on the coarsest level.  Returns
    (level models, A per level, prolongations, the V-cycle, the Krylov solver)."""
    from .. import linalg
    from .partition import levels_for

    levels = [HexTransientModel(fine.mesh, q, fine.materials, surfaces=fine.surfaces, pec=fine.pec, q1d=fine.q1d)
              for q in levels_for(fine.p)[:-1]] + [fine]
    for lv in levels[:-1]:
        lv.prepare(ctx, geom=fine.geom)
    A = [lv.system(a) for lv in levels]
    P = [linalg.Interp(ctx, c.nd, f.nd) for c, f in zip(levels[:-1], levels[1:])]
    coarse = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1.0e-2, max_it=8)
    gmg = linalg.gmg(ctx, A, P, coarse, cheby_order=max(2 * fine.p, 4))
    return levels, A, P, gmg, linalg.cg(ctx, A[-1], gmg, rel_tol=rel_tol, max_it=max_it)


# ---- the reference's coaxial example -----------------------------------------------------------------------------------------

C0_M_S = 299792458.0
MU0 = 4.0e-7 * np.pi
Z0_OHM = MU0 * C0_M_S
EPS0 = 1.0 / (MU0 * C0_M_S * C0_M_S)

# examples/coaxial/coaxial_matched.json
COAXIAL_MATCHED = dict(
    L0=1.0e-3, order=3,
    materials=[dict(attributes=[1], mu_r=1.0, eps_r=2.08, sigma=4.629e-2)],  # sigma in S/m
    pec=[2],
    ports=[dict(index=1, attributes=[3], R=50.0, direction=+1, excitation=True),
           dict(index=2, attributes=[4], R=50.0, direction=+1, excitation=False)],
    excitation="mod_gaussian", freq_ghz=10.0, width_ns=0.05, max_t_ns=1.0, dt_ns=0.005, rho_inf=1.0,
    linear=dict(tol=1.0e-8, max_it=100),
)


def _face_points(lf_axes, pts1d):
    """Reference points [q1d^2, 3] of a local face (nax, side, uax, vax), q = qu + q1d qv."""
    nax, side, uax, vax = lf_axes
    qv, qu = np.meshgrid(pts1d, pts1d, indexing="ij")
    X = np.zeros((pts1d.size ** 2, 3))
    X[:, nax], X[:, uax], X[:, vax] = float(side), qu.ravel(), qv.ravel()
    return X


def _rt_values_at(p, X):
    """RT reference basis [3, nq, P] at arbitrary reference points X [nq, 3] (tensor dof order of rthex)."""
    from .basis1d import gauss_legendre, gauss_lobatto, lagrange_eval
    from .rthex import rt_block_shape

    cn, on = gauss_lobatto(p + 1), gauss_legendre(p)[0]
    out = np.zeros((3, X.shape[0], 3 * p * p * (p + 1)))
    for comp in range(3):
        tabs = [lagrange_eval(cn if ax == comp else on, X[:, ax])[0] for ax in range(3)]  # [nq, n_ax]
        nx, ny, nz = rt_block_shape(p, comp)
        val = np.einsum("qk,qj,qi->qkji", tabs[2], tabs[1], tabs[0]).reshape(X.shape[0], nz * ny * nx)
        base = comp * p * p * (p + 1)
        out[comp, :, base:base + nx * ny * nz] = val
    return out


class CoaxialPort:
    """One coaxial lumped port (models/lumpedportoperator.cpp with fem/lumpedelement.cpp:139-179) on a set of boundary faces of a
    HexTransientModel's mesh, in mesh length units and impedances in units of Z0:
      centre, inner and outer radius from the port's nodes; L = ln(r_o / r_i), W = 2 pi, R_s = R W / L
      mode(x) = direction (x - x0) / |x - x0|^2   (r_hat / r)
      v: V = v . E = 1 / (2 pi) int E . r_hat / r dS                      (:210-231)
      s: the excitation vector int 2 H_inc mode . v dS, H_inc = 1 / sqrt(R_s W L)   (:628-662)
      Q: P = E^T Q B = int E . (n x mu^-1 B) dS, n the outward normal      (:234-292), I = P / V in a transient run
    """

    def __init__(self, model, face_mask, R_over_Z0, direction, mu_inv_of_attr):
        import scipy.sparse as sp

        from .basis1d import Tables1D
        from .fespace import NDHexBoundaryBlock
        from .mesh import HEX_FACE_AXES, _q2_1d

        mesh, nd, rt, p, q1d = model.mesh, model.nd, model.rt, model.p, model.q1d
        self.face_mask = face_mask
        blk = NDHexBoundaryBlock(nd, face_mask=face_mask)
        sint, sgrad, sw = blk.tables(q1d)
        pn = np.unique(blk.elem_nodes)
        lo, hi = mesh.x[pn].min(axis=0), mesh.x[pn].max(axis=0)
        self.x0 = x0 = 0.5 * (lo + hi)
        r = np.linalg.norm(mesh.x[pn] - x0, axis=1)
        self.r_inner, self.r_outer = float(r.min()), float(r.max())
        self.L, self.W = float(np.log(self.r_outer / self.r_inner)), 2.0 * np.pi
        self.R = float(R_over_Z0)
        self.Rs = self.R * self.W / self.L
        self.Hinc = 1.0 / np.sqrt(self.Rs * self.W * self.L)
        self.V_inc = np.sqrt(self.Rs / (self.W * self.L)) * self.L  # GetExcitationVoltage (:142-165)
        t = Tables1D(p, q1d)
        B2, _ = _q2_1d(t.qx)
        N = np.einsum("vb,ua->vuba", B2, B2).reshape(q1d * q1d, 9)  # node iu + 3 iv at q = qu + q1d qv
        Xe = blk.nodes[blk.elem_nodes]                                # [ne, 9, 3]
        xq = np.einsum("qn,eni->eqi", N, Xe)
        Js = np.einsum("dqn,eni->eqid", sgrad, Xe)                    # [ne, Q, 3, 2]
        G = np.einsum("eqia,eqib->eqab", Js, Js)
        dS = np.sqrt(np.linalg.det(G)) * sw[None, :]
        Jpinv = np.einsum("eqia,eqab->eqib", Js, np.linalg.inv(G))    # J (J^T J)^-1: covariant map of the tangential basis
        d = xq - x0
        mode = direction * d / np.sum(d * d, axis=2, keepdims=True)
        sign = np.where(blk.orients, -1.0, 1.0)
        # phi_i(q) in physical space [ne, Q, 3, P]
        phi = np.einsum("eqia,aqj->eqij", Jpinv, sint) * sign[:, None, None, :]
        lf = np.einsum("eq,eqi,eqij->ej", dS, mode, phi)
        form = np.zeros(nd.ndofs)
        np.add.at(form, blk.offsets.ravel(), lf.ravel())
        self.v = form / self.W
        self.s = 2.0 * self.Hinc * form
        # the power form: E . (n x H), H = mu^-1 B of the adjacent element at the face points
        bmask = face_mask[mesh.elem_faces]
        rows, cols, vals = [], [], []
        e0 = 0
        for lfi, axes in enumerate(HEX_FACE_AXES):
            el = np.nonzero(bmask[:, lfi])[0]
            if el.size == 0:
                continue
            nax, side, uax, vax = axes
            X = _face_points(axes, t.qx)
            Jv = mesh.jacobian_at(X)[el]                               # [n, Q, 3, 3]
            det = np.linalg.det(Jv)
            nrm = np.cross(Jv[..., uax], Jv[..., vax])                 # parallel to the normal; orient it outward
            out_dir = (1.0 if side else -1.0) * Jv[..., nax]
            nrm *= np.sign(np.sum(nrm * out_dir, axis=2))[..., None]
            nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
            rtv = _rt_values_at(p, X)                                  # [3, Q, P_rt]
            rsign = rt.elem_sign_lex[el].astype(np.float64)
            muinv = np.array([mu_inv_of_attr[a] for a in mesh.attr[el]])
            Hb = np.einsum("e,eqid,dqj->eqij", muinv, Jv, rtv) / det[..., None, None] * rsign[:, None, None, :]
            nxH = np.cross(nrm[..., None, :], np.moveaxis(Hb, 2, 3))   # [n, Q, P_rt, 3]
            sl = slice(e0, e0 + el.size)
            assert np.array_equal(blk.faces[sl], mesh.elem_faces[el, lfi])
            loc = np.einsum("eq,eqin,eqmi->enm", dS[sl], phi[sl], nxH)  # [n, P_nd_face, P_rt]
            rows.append(np.repeat(blk.offsets[sl][:, :, None], loc.shape[2], axis=2).ravel())
            cols.append(np.repeat(rt.elem_dof_lex[el][:, None, :], loc.shape[1], axis=1).ravel())
            vals.append(loc.ravel())
            e0 += el.size
        self.Q = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nd.ndofs, rt.ndofs)).tocsr()
        self.Q.eliminate_zeros()


class TransientReferenceSystem:
    """A transient configuration as the reference defines it (drivers/transientsolver.cpp, models/spaceoperator.cpp,
    models/timeoperator.cpp) on a hexahedral mesh, in mesh length units: times in units of L0 / c0, impedances in units of Z0,
    conductivities in units of 1 / (Z0 L0) -- the reference's nondimensionalisation with Lc = L0 (utils/units.hpp); the
    measurements are dimensionalised as it does (Hc^2 Z0 Lc^2 = 1 W: volts = sqrt(Z0), amperes = 1 / sqrt(Z0), joules = tc).
      K   curl-curl with mu^-1                   M   mass with eps
      C   volume mass with sigma + 1 / R_s surface masses on the lumped-port faces
      PEC on cfg["pec"] (K, C: DIAG_ZERO, M: DIAG_ONE), the excitation vector of the excited port
    measure(t, E, B): V_j, I_j = P_j / V_j of every port, V_inc, I_inc of the excited one, E_elec, E_mag.
    ctx given: the device operators, A(a) as one fused operator per level of the p-hierarchy [1, 2, .., order], and PCG with the
    p-multigrid V-cycle (plain Chebyshev smoothing, Jacobi-PCG on the coarsest level) as KspSolver configures an SPD problem."""

    def __init__(self, ctx, mesh, cfg=COAXIAL_MATCHED):
        self.cfg, self.mesh, self.ctx = cfg, mesh, ctx
        p = self.p = cfg["order"]
        L0 = cfg["L0"]
        self.tc_ns = 1.0e9 * L0 / C0_M_S
        self.dt = cfg["dt_ns"] / self.tc_ns
        self.nsteps = int(round(cfg["max_t_ns"] / cfg["dt_ns"]))
        self.rho_inf = cfg["rho_inf"]
        self.kind = cfg["excitation"]
        self.omega = 2.0 * np.pi * cfg["freq_ghz"] * self.tc_ns
        self.tau = cfg["width_ns"] / self.tc_ns
        self.t0 = pulse_delay(self.kind, self.tau)
        nattr = int(mesh.attr.max())
        attr_mat = [-1] * nattr
        for k, m in enumerate(cfg["materials"]):
            for a in m["attributes"]:
                attr_mat[a - 1] = k
        sig = [m.get("sigma", 0.0) * Z0_OHM * L0 for m in cfg["materials"]]
        self.materials = dict(attr_mat=attr_mat, eps=[m["eps_r"] for m in cfg["materials"]],
                              mu_inv=[1.0 / m["mu_r"] for m in cfg["materials"]], sigma=sig if any(sig) else None)
        fid = boundary_face_ids(mesh, mesh.bdr_faces)

        def faces(attrs):
            mask = np.zeros(mesh.nfaces, dtype=bool)
            mask[fid[np.isin(mesh.bdr_attr, attrs)]] = True
            return mask

        self.pec = faces(cfg["pec"])
        port_masks = [faces(pt["attributes"]) for pt in cfg["ports"]]
        geo = HexTransientModel(mesh, p, self.materials, pec=self.pec)  # (spaces for the port geometry)
        mu_of_attr = {a + 1: self.materials["mu_inv"][k] for a, k in enumerate(attr_mat) if k >= 0}
        self.ports = [CoaxialPort(geo, m, pt["R"] / Z0_OHM, pt["direction"], mu_of_attr) for m, pt in zip(port_masks, cfg["ports"])]
        self.surfaces = [(pt.face_mask, 1.0 / pt.Rs) for pt in self.ports]
        self.model = HexTransientModel(mesh, p, self.materials, surfaces=self.surfaces, pec=self.pec)
        self.excited = [j for j, pt in enumerate(cfg["ports"]) if pt["excitation"]]
        assert len(self.excited) == 1, "a transient run takes one excitation"
        self.negJ = self.ports[self.excited[0]].s.copy()
        self.negJ[self.model.ess] = 0.0
        self.nE, self.nB = self.model.nE, self.model.nB

    # -- time dependence ---------------------------------------------------------------------------------------------------
    def g(self, t):
        return float(pulse_value(self.kind, t, self.omega, self.tau, self.t0))

    def dg(self, t):
        return float(pulse_derivative(self.kind, t, self.omega, self.tau, self.t0))

    # -- measurements (numpy vectors) ------------------------------------------------------------------------------------------
    def measure(self, t, E, B, M_eps=None, M_mu=None):
        cpu = self.model.cpu()
        M_eps = cpu["M_eps"] if M_eps is None else M_eps
        M_mu = cpu["M_mu"] if M_mu is None else M_mu
        vs, cs = np.sqrt(Z0_OHM), 1.0 / np.sqrt(Z0_OHM)
        row = dict(t_ns=t * self.tc_ns)
        g = self.g(t)
        ex = self.ports[self.excited[0]]
        V_inc = ex.V_inc * g
        row["V_inc1"] = V_inc * vs
        row["I_inc1"] = (g * g / V_inc if abs(V_inc) > 0.0 else 0.0) * cs
        for j, pt in enumerate(self.ports):
            V = float(pt.v @ E)
            P = float(E @ (pt.Q @ B))
            row[f"V{j + 1}"] = V * vs
            row[f"I{j + 1}"] = (P / V if abs(V) > 0.0 else 0.0) * cs
        row["E_elec"] = 0.5 * float(E @ (M_eps @ E)) * 1.0e-9 * self.tc_ns
        row["E_mag"] = 0.5 * float(B @ (M_mu @ B)) * 1.0e-9 * self.tc_ns
        return row

    COLUMNS = ("V_inc1", "V1", "V2", "I_inc1", "I1", "I2", "E_elec", "E_mag")

    def run_reference(self):
        """The whole run through reference_steps: {column: [nsteps + 1]}."""
        cpu = self.model.cpu()
        nE = self.nE
        rows = reference_steps(cpu["K"], cpu["C"], cpu["M"], cpu["Curl"], self.negJ, self.dg, self.rho_inf, self.dt, self.nsteps,
                               observe=lambda step, t, u: self.measure(t, u[nE:2 * nE], u[2 * nE:]))
        return {k: np.array([r[k] for r in rows]) for k in ("t_ns",) + self.COLUMNS}


    # -- device ---------------------------------------------------------------------------------------------------------------
    def build_device(self, a=None, rel_tol=None, max_it=None):
        """Operators, A(a) on every level of the p-hierarchy, the solvers and the stepper (a: the stage factor of this run)."""
        import torch

        from .. import linalg

        ctx, cfg = self.ctx, self.cfg
        a = stage_factor(self.rho_inf, self.dt) if a is None else a
        rel_tol = cfg["linear"]["tol"] if rel_tol is None else rel_tol
        max_it = cfg["linear"]["max_it"] if max_it is None else max_it
        fine = self.model
        self.dev = dev = fine.device(ctx)
        self.levels, self.A, self.P, self.gmg, self.a_solver = pmg_system_solver(ctx, fine, a, rel_tol, max_it)
        self.m_solver = linalg.cg(ctx, dev["M"], linalg.jacobi(ctx, dev["M"]), rel_tol=rel_tol, max_it=max_it)
        to_dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
        self.pulse = linalg.pulse(self.kind, omega=self.omega, tau=self.tau, t0=self.t0)
        self.time_op = linalg.TimeOperator(ctx, dev["K"], dev["C"], dev["Curl"], self.m_solver, self.a_solver, to_dev(self.negJ),
                                           self.pulse, self.rho_inf, self.dt)
        self._dev_ports = []
        for pt in self.ports:
            Q = pt.Q.tocoo()
            rows, cols = np.unique(Q.row), np.unique(Q.col)
            sub = pt.Q[rows][:, cols].toarray()
            self._dev_ports.append((to_dev(pt.v), to_dev(rows.astype(np.int64)), to_dev(cols.astype(np.int64)), to_dev(sub)))
        self._tmp = (torch.empty(self.nE, dtype=torch.float64, device="cuda"), torch.empty(self.nB, dtype=torch.float64, device="cuda"))
        return self.time_op

    def measure_device(self, t):
        """measure() on the stepper's device state: the energies through the device mass operators (Nedelec with eps,
        Raviart-Thomas with mu^-1), the port forms as dot products."""
        T = self.time_op
        E, B = T.E, T.B
        vs, cs = np.sqrt(Z0_OHM), 1.0 / np.sqrt(Z0_OHM)
        row = dict(t_ns=t * self.tc_ns)
        g = self.g(t)
        V_inc = self.ports[self.excited[0]].V_inc * g
        row["V_inc1"] = V_inc * vs
        row["I_inc1"] = (g * g / V_inc if abs(V_inc) > 0.0 else 0.0) * cs
        for j, (v, rows, cols, sub) in enumerate(self._dev_ports):
            V = float(v @ E)
            P = float(E[rows] @ (sub @ B[cols]))
            row[f"V{j + 1}"] = V * vs
            row[f"I{j + 1}"] = (P / V if abs(V) > 0.0 else 0.0) * cs
        # (the operators gather their input entry by entry: the views of the state's blocks serve as they are, whatever nE)
        tE, tB = self._tmp
        row["E_elec"] = 0.5 * float(E @ self.dev["M_eps"].mult(E, tE)) * 1.0e-9 * self.tc_ns
        row["E_mag"] = 0.5 * float(B @ self.dev["M_mu"].mult(B, tB)) * 1.0e-9 * self.tc_ns
        return row

    def run_device(self, keep_states=False):
        """Init, then nsteps steps, measuring after each: {column: [nsteps + 1]} (and the states on request)."""
        T = self.time_op
        T.init(0.0)
        rows, states = [self.measure_device(0.0)], []
        for _ in range(self.nsteps):
            t = T.step()
            rows.append(self.measure_device(t))
            if keep_states:
                states.append(T.state().cpu().numpy().copy())
        out = {k: np.array([r[k] for r in rows]) for k in ("t_ns",) + self.COLUMNS}
        return (out, np.array(states)) if keep_states else out


def regression_close(a, b, rtol=2.0e-2, atol=1.0e-11):
    """The reference's regression rule (test/unit/regression_helpers.cpp:267): |a - b| <= max(atol, rtol max(|a|, |b|))."""
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b) <= np.maximum(atol, rtol * np.maximum(np.abs(a), np.abs(b)))
