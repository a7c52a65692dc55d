"""Operators, transfers and solvers on hanging-node spaces ACROSS ranks: every rank is a thread over linalg.LocalGroup with its
fem/ncpart.py view and a Conforming that carries the halo (pa_conform_create_dist).  Operators and transfers against the
oracle's classes with the global scipy P at the rank's owned dofs; solves against the same solve on one rank (the gates of
tests/test_multirank_local_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from tests import nc_ranks_util as ru  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import util  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


_refs = {}


def _operator_reference(name, kind, p):
    """Oracle results on global true-dof vectors, once per case (shared by the worlds)."""
    key = (name, kind, p)
    if key in _refs:
        return _refs[key]
    s = nu.nc_space(name, kind, p)
    q1d = p + 1
    if kind == "nd":
        cm, bm = util.make_ctx("scalar", 2)
        cc, bc = util.make_ctx("identity")
        oA = nu.ConstrainedParOperatorOracle([nu.CLocal(s, np.concatenate([bm, bc]), q1d, cm, cc)], s.prolongation(), s.ess_dofs())
    else:
        c_mass = po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([2.08])], dim=1)
        c_diff = util.make_ctx("identity")[0]
        oA = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hcurlmass", c_mass, c_diff, q1d)], s.prolongation(), s.ess_dofs())
    rng = np.random.default_rng(p)
    x, y0 = rng.uniform(-1, 1, s.n_true), rng.uniform(-1, 1, s.n_true)
    _refs[key] = dict(x=x, y0=y0, mult=oA.mult(x), add_mult=oA.add_mult(x, y0, -0.5), eliminate_rhs=oA.eliminate_rhs(x, y0),
                      diagonal=oA.diagonal())
    return _refs[key]


def _local_operator(view, kind, q1d):
    geom = ceed.GeomFactorData(view.mesh, q1d)
    if kind == "nd":
        bm, bc = util.make_ctx("scalar", 2)[1], util.make_ctx("identity")[1]
        return ceed.curlcurlmass_operator(geom, view, bm, bc), geom
    c_mass = po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([2.08])], dim=1)
    return ceed.diffusionmass_operator(geom, view, c_mass.pack(), util.make_ctx("identity")[0].pack()), geom


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name,kind,p", [("A", "nd", 1), ("A", "nd", 2), ("A", "nd", 3), ("C", "nd", 2), ("A", "h1", 2)])
def test_par_operator_across_ranks(name, kind, p, world):
    """Mult, MultTranspose, AddMult, EliminateRHS, AssembleDiagonal (and Mult in place) on each rank's owned dofs."""
    ref = _operator_reference(name, kind, p)
    s, vs = ru.views(name, kind, p, f"rcb{world}")

    def rank_main(ctx, rank):
        v = vs[rank]
        own = v.l2g[:v.n_true]
        conf, halo = ru.rank_conforming(ctx, v, world)
        local, geom = _local_operator(v, kind, p + 1)
        A = linalg.ParOperator(ctx, local, v.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
        assert A.n == v.n_true and not A.fuses_essential() and not A.prepare_cheby_step()
        x, y0, n = ref["x"][own], ref["y0"][own], v.n_true
        err = dict(mult=_rel(A.mult(_dev(x), _new(n)).cpu().numpy(), ref["mult"][own]),
                   mult_transpose=_rel(A.mult_transpose(_dev(x), _new(n)).cpu().numpy(), ref["mult"][own]),
                   add_mult=_rel(A.add_mult(_dev(x), _dev(y0), -0.5).cpu().numpy(), ref["add_mult"][own]),
                   eliminate_rhs=_rel(A.eliminate_rhs(_dev(x), _dev(y0)).cpu().numpy(), ref["eliminate_rhs"][own]),
                   diagonal=_rel(A.assemble_diagonal(_new(n)).cpu().numpy(), ref["diagonal"][own]))
        xy = _dev(x)
        err["in_place"] = _rel(A.mult(xy, xy).cpu().numpy(), ref["mult"][own])
        print(rank, " ".join(f"{k} {e:.2e}" for k, e in err.items()))
        assert max(err.values()) < 1e-12, (rank, err)
        with pytest.raises(Exception, match="halo"):
            A.parallel_assemble()
        return v.n_true

    assert sum(ru.run_ranks(world, rank_main)) == s.n_true


@pytest.mark.parametrize("world", [2, 4])
def test_complex_par_operator_across_ranks(world):
    """(K + M) + i M on mesh A at order 2: both parts."""
    s, vs = ru.views("A", "nd", 2, f"rcb{world}")
    cm, bm = util.make_ctx("scalar", 2)
    cc, bc = util.make_ctx("identity")
    P, ess = s.prolongation(), s.ess_dofs()
    oR = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hdivmass", cm, cc, 3)], P, ess, po.DIAG_ONE)
    oI = nu.ConstrainedParOperatorOracle([nu.oracle_local(s, "hcurl", cm, None, 3)], P, ess, po.DIAG_ZERO)
    rng = np.random.default_rng(4)
    xr, xi = rng.uniform(-1, 1, s.n_true), rng.uniform(-1, 1, s.n_true)
    wr, wi = oR.mult(xr) - oI.mult(xi), oI.mult(xr) + oR.mult(xi)

    def rank_main(ctx, rank):
        v = vs[rank]
        own, n = v.l2g[:v.n_true], v.n_true
        conf, halo = ru.rank_conforming(ctx, v, world)
        geom = ceed.GeomFactorData(v.mesh, 3)
        Ar, Ai = ceed.curlcurlmass_operator(geom, v, bm, bc), ceed.ndmass_operator(geom, v, bm)
        A = linalg.ComplexParOperator(ctx, Ar, Ai, v.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
        yr, yi = A.mult(_dev(xr[own]), _dev(xi[own]), _new(n), _new(n))
        assert _rel(yr.cpu().numpy(), wr[own]) < 1e-12 and _rel(yi.cpu().numpy(), wi[own]) < 1e-12

    ru.run_ranks(world, rank_main)


@pytest.mark.parametrize("world", [2, 4])
def test_transfers_across_ranks(world):
    """Interp 1 -> 2 and 2 -> 3 and the discrete gradient at order 2 on mesh C, with their transposes, against the global
    R_f I P_c; the adjoint identity through global dots."""
    how = f"rcb{world}"
    sp = [nu.nc_space("C", "nd", p) for p in (1, 2, 3)]
    vw = [ru.views("C", "nd", p, how)[1] for p in (1, 2, 3)]
    h1, vh = ru.views("C", "h1", 2, how)
    rng = np.random.default_rng(6)
    cases = []
    for a, b in zip(sp[:-1], sp[1:]):
        I = po.InterpOracle(a.elem_dof_lex, a.elem_sign_lex, b.elem_dof_lex, b.elem_sign_lex, a.ndofs, b.ndofs,
                            po.nd_hex_interp_lex(a.p, b.p))
        Pc = a.prolongation()
        xc, xf = rng.uniform(-1, 1, a.n_true), rng.uniform(-1, 1, b.n_true)
        cases.append((xc, xf, I.mult(Pc @ xc)[:b.n_true], Pc.T @ I.mult_transpose(np.concatenate([xf, np.zeros(b.n_local - b.n_true)]))))
    nd = sp[1]
    Gl = nu.local_gradient(h1, nd)
    xh, xn = rng.uniform(-1, 1, h1.n_true), rng.uniform(-1, 1, nd.n_true)
    cases.append((xh, xn, (Gl @ (h1.prolongation() @ xh))[:nd.n_true],
                  h1.prolongation().T @ (Gl.T @ np.concatenate([xn, np.zeros(nd.n_local - nd.n_true)]))))

    def rank_main(ctx, rank):
        doms = [vw[0][rank], vw[1][rank], vh[rank]]
        rngs = [vw[1][rank], vw[2][rank], vw[1][rank]]
        keep = []
        for k, (vc, vf) in enumerate(zip(doms, rngs)):
            conf, halo = ru.rank_conforming(ctx, vc, world)
            T = (linalg.Gradient if k == 2 else linalg.Interp)(ctx, vc, vf, conforming=conf)
            keep.append((conf, halo, T))
            xc, xf, wf, wc = cases[k]
            oc, of = vc.l2g[:vc.n_true], vf.l2g[:vf.n_true]
            dxc, dxf = _dev(xc[oc]), _dev(xf[of])
            yf = T.mult(dxc, _new(vf.n_true))
            yc = T.mult_transpose(dxf, _new(vc.n_true))
            assert _rel(yf.cpu().numpy(), wf[of]) < 1e-13 and _rel(yc.cpu().numpy(), wc[oc]) < 1e-13, (rank, k)
            lhs, rhs = ctx.dot(dxf, yf), ctx.dot(dxc, yc)
            assert abs(lhs - rhs) < 1e-12 * abs(lhs), (rank, k, lhs, rhs)
            assert abs(lhs - xf @ wf) < 1e-12 * abs(lhs)

    ru.run_ranks(world, rank_main)


# ---- solvers on the refined cylinder ------------------------------------------------------------------------------------

_solves = {}


def _solve(world, which):
    """which: 'jacobi' (Jacobi-PCG at order 2) or 'gmg' (PCG + p-multigrid [1, 2, 3], Chebyshev smoothing, Jacobi-PCG at level
    0), rel_tol 1e-9; world 1 takes the same path with an empty halo."""
    key = (world, which)
    if key in _solves:
        return _solves[key]
    levels = [2] if which == "jacobi" else [1, 2, 3]
    how = f"rcb{world}"
    vw = [ru.views("C", "nd", p, how)[1] for p in levels]
    n_glob = nu.nc_space("C", "nd", levels[-1]).n_true
    bm, bc = util.make_ctx("scalar", 2)[1], util.make_ctx("identity")[1]

    def rank_main(ctx, rank):
        vs = [v[rank] for v in vw]
        geom = ceed.GeomFactorData(vs[0].mesh, levels[-1] + 1)
        fine = ceed.curlcurlmass_operator(geom, vs[-1], bm, bc)
        local = [fine.coarsen(geom, v) for v in vs[:-1]] + [fine]
        confs = [ru.rank_conforming(ctx, v, world) for v in vs]
        A = [linalg.ParOperator(ctx, op, v.ess_dofs(), linalg.DIAG_ONE, conforming=c[0]) for op, v, c in zip(local, vs, confs)]
        if which == "jacobi":
            B = linalg.jacobi(ctx, A[-1])
        else:
            P = [linalg.Interp(ctx, a, b, conforming=c[0]) for a, b, c in zip(vs[:-1], vs[1:], confs[:-1])]
            coarse = linalg.cg(ctx, A[0], linalg.jacobi(ctx, A[0]), rel_tol=1e-3, max_it=200)
            B = linalg.gmg(ctx, A, P, coarse, cheby_order=6)
        n = vs[-1].n_true
        b = A[-1].mult(_dev(np.ones(n)), _new(n))
        b[torch.from_numpy(vs[-1].ess_dofs().astype(np.int64)).cuda()] = 0.0
        K = linalg.cg(ctx, A[-1], B, rel_tol=1e-9, max_it=600)
        x = K.mult(b, _new(n))
        st = K.stats()
        Ab, Ax = A[-1].mult(b, _new(n)), A[-1].mult(x, _new(n))
        return dict(st, n=n, bb=ctx.dot(b, b), bAb=ctx.dot(b, Ab), xx=ctx.dot(x, x), xAx=ctx.dot(x, Ax))

    out = ru.run_ranks(world, rank_main, timeout=300)
    res = dict(out[0])
    res["n"] = sum(o["n"] for o in out)
    for o in out[1:]:  # the reductions are global: every rank holds the same values
        for k in ("bb", "bAb", "xx", "xAx", "iterations"):
            assert o[k] == out[0][k], (k, o[k], out[0][k])
    assert res["n"] == n_glob
    _solves[key] = res
    return res


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("which", ["jacobi", "gmg"])
def test_solves_across_ranks_match_one_rank(which, world):
    one, many = _solve(1, which), _solve(world, which)
    print(which, world, one, many)
    assert one["converged"] and many["converged"] and many["n"] == one["n"]
    assert abs(many["iterations"] - one["iterations"]) <= 1, (many["iterations"], one["iterations"])
    for k in ("bb", "bAb"):   # operator applies: rounding only
        assert abs(many[k] - one[k]) < 1e-11 * abs(one[k]), (k, many[k], one[k])
    for k in ("xx", "xAx"):   # solves to 1e-9
        assert abs(many[k] - one[k]) < 1e-6 * abs(one[k]), (k, many[k], one[k])


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_assembled_forms_refuse_a_distributed_conforming():
    """parallel_assemble and rap_conforming with a Conforming that carries a halo: an assembled level across ranks is not
    built."""
    s = nu.nc_space("A", "nd", 1)
    ctx = linalg.Context()
    conf = linalg.Conforming(ctx, s, n_shared=s.n_true)
    local = ceed.ndmass_operator(ceed.GeomFactorData(s.mesh, 2), s, util.make_ctx("identity")[1])
    A = linalg.ParOperator(ctx, local, s.ess_dofs(), linalg.DIAG_ONE, conforming=conf)
    with pytest.raises(Exception, match="halo"):
        A.parallel_assemble()
    csr = local.full_assemble_device()
    with pytest.raises(Exception, match="halo"):
        linalg.rap_conforming(ctx, csr, conf, conf)
    with pytest.raises(Exception, match="halo"):
        linalg.rap_conforming(ctx, csr, None, conf)
