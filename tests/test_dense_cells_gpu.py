"""Every reachable instantiation of the dense MFMA element kernels (palace_amd/csrc/pa_dense.hip) against the oracle: one case per
cell of tests/dense_cases.py.  Each case builds its operator, asserts through `Operator.dense_kernel()` that it landed in the stated
cell (a case that drifts to another kernel fails), and compares with `po.CeedOperatorOracle` on the same arrays: `Mult` into a
prefilled y (dofs no element touches come back 0), `AddMult`, the masked apply after `set_essential`, and the assembled diagonal
(`dense_diag_kernel` for the 3-D modes, `dense_diag_qd_kernel` for the others).  Where the affine form runs, the general form on the
same elements agrees to 1e-14; the staged cases under PALACE_AMD_DENSE=staged are built a second time without it (resident) and
compared with the oracle again; the split-vector cases give the bits of the plain apply; the complex cases are compared with the
four real oracle applies.

Tolerance: the project's REL = 1e-12 of max |ref| (tests/test_dense_gpu.py, tests/test_tet_gpu.py) in every case."""
import ctypes as C

import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import dense_cases as dc

pytestmark = pytest.mark.gpu
REL = 1e-12


def _spd(rng, d):
    A = rng.uniform(-1, 1, (d, d))
    return A @ A.T + 2.0 * np.eye(d)


def _context(letter, sdim, seed, nonsym=False):
    rng = np.random.default_rng(seed)
    if letter == "1":
        return po.CoeffCtx(attr_mat=[1, 0], mat_coeff=[np.array([1.9]), np.array([0.4])], dim=1)
    m = rng.uniform(-1, 1, (sdim, sdim)) + 3.0 * np.eye(sdim) if nonsym else _spd(rng, sdim)
    return po.CoeffCtx(attr_mat=[0, 1], mat_coeff=[m, np.array([0.6])], a=1.2, dim=sdim)


def _oracle_geom(case, I):
    ne, Q = I.J.shape[:2]
    attr = I.attr.astype(np.float64)
    Jcm = np.transpose(I.J, (0, 1, 3, 2)).reshape(ne, Q, -1)  # column-major
    if case.dim == 3:
        return po.build_geom_factor_33(attr, I.w, Jcm)
    if case.dim == 2:
        return (po.build_geom_factor_32 if case.sdim == 3 else po.build_geom_factor_22)(attr, I.w, Jcm)
    return po.build_geom_factor_line(attr, I.w, I.J[..., 0])


class _Built:
    pass


def _describe(case, I, mode=None):
    """The library's arguments and the oracle of one operator on the inputs of a case (`mode`: another mode on the same block, the
    imaginary part of the complex form)."""
    from palace_amd import ceed

    c = case if mode is None else dc.Case(case.id, "resident", case.PT, mode, case.geo, case.P, case.Q, case.ne, 3, 3, case.restr)
    lib_qf, orc_qf, ops_s, ctx_s = dc.qfunction(c)
    vec = dc.MODE_INFO[c.mode][0] or bool(c.hdiv)
    ctxs = [_context(l, c.sdim, 11 + 7 * k + (100 if mode else 0), nonsym=(c.staged_by == "nonsym" and l == "M")) for k, l in enumerate(ctx_s)]
    B = _Built()
    B.blob = np.concatenate([x.pack() for x in ctxs])
    B.qf = getattr(ceed, lib_qf)
    B.ops = sum({"I": ceed.EVAL_INTERP, "G": ceed.EVAL_GRAD, "C": ceed.EVAL_CURL, "D": ceed.EVAL_DIV, "W": ceed.EVAL_WEIGHT}[l] for l in ops_s)
    P, Q = I.offsets.shape[1], len(I.w)
    n_i, n_d = dc.table_shapes(c)  # (the tables of a complex case hold both kinds; each of its operators reads its own)
    interp, deriv = (I.interp if n_i else None), (I.deriv if n_d else None)
    B.fe = ceed.FE_HDIV if c.hdiv else (ceed.FE_HCURL if vec else ceed.FE_H1)
    B.interp, B.deriv = interp, deriv
    div = c.hdiv in ("divdiv", "divdivmass")
    dcomp = 1 if div or (c.dim == 2 and vec) else c.dim
    o_interp = interp if interp is not None else np.zeros((c.dim if vec else 1, Q, P))
    o_deriv = deriv if deriv is not None else (interp if (c.hdiv == "mass" and c.dim == 3) else np.zeros((dcomp, Q, P)))
    kw = {}
    if "W" in ops_s:
        kw["qw"] = I.w
    if div:
        kw["deriv_comps"] = 1
    if I.curl_orients is not None:
        kw["curl_orients"] = I.curl_orients
    B.oracle = lambda og: po.CeedOperatorOracle(I.lsize, I.offsets, I.orients, o_interp, o_deriv, og, getattr(po, orc_qf), *ctxs,  # noqa: E731
                                                vector_fe=vec, **kw)
    return B


def _make(I, geom, B):
    from palace_amd import ceed

    block = ceed.DenseBlock(B.fe, I.lsize, I.offsets, B.interp, B.deriv, orients=I.orients, curl_orients=I.curl_orients)
    return ceed.Operator(I.lsize, I.lsize).add_dense_integrator(geom, block, B.qf, B.blob, B.ops).finalize()


def _assert_cell(op, case, form=None, geo=None):
    k = op.dense_kernel()
    form, geo = form or case.form, geo or case.geo
    want = dict(PT=case.PT, mode=dc.MODES.index(case.mode), resident=form != "staged",
                geometry={"curved": 0, "affine": 1, "list": 2, "-": 0}[geo], lists=case.lists if geo == "list" else (0, 0),
                rows=case.rows, split=k["split"])
    assert k == want, (case.id, k, want)
    if form == "split":
        assert k["split"]
    return k


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _err(got, ref, what, case):
    e = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{case.id}: {what} {e:.2e}")
    return e


@pytest.mark.parametrize("case", dc.CASES, ids=[c.id for c in dc.CASES])
def test_dense_cell(case, monkeypatch):
    import torch

    from palace_amd import ceed, lib

    I = dc.inputs(case)
    geom = ceed.DenseGeomFactorData(I.elem_nodes, I.nodes, I.attr, I.grad, I.w)
    og = _oracle_geom(case, I)
    B = _describe(case, I)
    if case.staged_by == "env":
        monkeypatch.setenv("PALACE_AMD_DENSE", "staged")
    op = _make(I, geom, B)
    monkeypatch.delenv("PALACE_AMD_DENSE", raising=False)
    _assert_cell(op, case)
    orc = B.oracle(og)
    n = I.lsize
    rng = np.random.default_rng(len(case.id) + case.P)
    x = rng.uniform(-1, 1, n)
    ref = orc.apply_add(x, np.zeros(n))
    scale = np.abs(ref).max()
    xd = _dev(x)
    # Mult into a prefilled y
    y = op.mult(xd, torch.full((n,), 7.0, dtype=torch.float64, device="cuda")).cpu().numpy()
    assert _err(y, ref, "Mult", case) < REL
    assert np.all(y[~I.touched] == 0.0)
    # AddMult
    y0 = rng.uniform(-1, 1, n)
    ya = op.add_mult(xd, _dev(y0)).cpu().numpy()
    assert np.abs(ya - (y0 + ref)).max() / scale < REL
    assert np.all(ya[~I.touched] == y0[~I.touched])
    if case.form == "complex":
        _complex(case, I, geom, og, op, orc, rng)
        return
    if case.form == "split":
        _split(case, I, geom, B, op, xd)
        return
    # diagonal
    dref = orc.diagonal()
    d = op.assemble_diagonal(torch.full((n,), 3.0, dtype=torch.float64, device="cuda")).cpu().numpy()
    assert _err(d, dref, "diagonal", case) < REL
    # masked apply: the listed entries of x read as zero (the rows of y are not fixed here)
    tdofs = np.nonzero(I.touched)[0]
    ess = np.sort(np.concatenate([rng.choice(tdofs, size=max(1, tdofs.size // 7), replace=False), np.nonzero(~I.touched)[0][:2]])).astype(np.int32)
    op.set_essential(ess)
    xm = x.copy()
    xm[ess] = 0.0
    refm = orc.apply_add(xm, np.zeros(n))
    ym = torch.full((n,), 5.0, dtype=torch.float64, device="cuda")
    lib.check(lib.load().pa_op_mult_essential(op.handle, C.c_void_p(xd.data_ptr()), C.c_void_p(ym.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.abs(ym.cpu().numpy() - refm).max() / scale < REL
    y2 = op.mult(xd, torch.empty_like(xd)).cpu().numpy()  # the plain apply still reads every entry
    assert np.array_equal(y2, y)
    # the general form on the same elements where the affine form ran
    if case.geo in ("affine", "list"):
        monkeypatch.setenv("PALACE_AMD_DENSE_AFFINE", "0")
        op_g = _make(I, geom, B)
        monkeypatch.delenv("PALACE_AMD_DENSE_AFFINE")
        _assert_cell(op_g, case, geo="curved")
        yg = op_g.mult(xd, torch.empty_like(xd)).cpu().numpy()
        e = np.abs(yg - y).max() / np.abs(y).max()
        print(f"{case.id}: affine vs general {e:.2e}")
        assert e <= 1e-14
    # the resident form of the same block where the switch forced the staged one
    if case.staged_by == "env":
        op_r = _make(I, geom, B)
        _assert_cell(op_r, case, form="resident", geo="curved")
        yr = op_r.mult(xd, torch.full((n,), 7.0, dtype=torch.float64, device="cuda")).cpu().numpy()
        assert _err(yr, ref, "Mult (resident twin)", case) < REL


def _split(case, I, geom, B, op, xd):
    """op.mult_split on (true, ghost) pieces against op.mult on the whole vector, bit for bit (tests/test_split_gpu.py): the ghost
    input in the second of two buffers with the first one poisoned, then essential dofs fused and their rows fixed."""
    import torch

    n = I.lsize
    assert op.supports_split()
    ref = op.mult(xd, torch.empty_like(xd))
    for n_true in (n, int(0.7 * n)):
        ng = n - n_true
        xg0 = torch.full((max(ng, 1),), float("nan"), dtype=torch.float64, device="cuda")
        xg1 = xd[n_true:].clone() if ng else torch.zeros(1, dtype=torch.float64, device="cuda")
        sel = torch.tensor([7], dtype=torch.int64, device="cuda")
        y, yg = torch.empty(n_true, dtype=torch.float64, device="cuda"), torch.zeros(max(ng, 1), dtype=torch.float64, device="cuda")
        op.mult_split(xd[:n_true].clone(), xg0, y, yg, xg1=xg1, sel=sel)
        assert torch.equal(y, ref[:n_true]), (case.id, n_true)
        if ng:
            assert torch.equal(yg, ref[n_true:]), (case.id, n_true)
    n_true = int(0.7 * n)
    ess = np.sort(np.random.default_rng(3).choice(n_true, size=max(1, n_true // 7), replace=False)).astype(np.int32)
    op2 = _make(I, geom, B)
    _assert_cell(op2, case)
    op2.set_essential(ess)
    ie = torch.from_numpy(ess.astype(np.int64)).cuda()
    xm = xd.clone()
    xm[ie] = 0.0
    refm = op.mult(xm, torch.empty_like(xd))
    for policy in (1, 0):
        want = refm.clone()
        want[ie] = xd[ie] if policy else 0.0
        y, yg = torch.empty(n_true, dtype=torch.float64, device="cuda"), torch.zeros(n - n_true, dtype=torch.float64, device="cuda")
        op2.mult_split(xd[:n_true].clone(), xd[n_true:].clone(), y, yg, ess_policy=policy)
        assert torch.equal(y, want[:n_true]) and torch.equal(yg, want[n_true:]), (case.id, policy)


def _complex(case, I, geom, og, op_r, orc_r, rng):
    """ComplexParOperator::Mult (one pass over the element data) against the four real oracle applies (linalg/operator.cpp:98-134),
    without and with essential dofs (inputs read as zero, rows set to x: DIAG_ONE)."""
    import torch

    from palace_amd import ceed, linalg

    Bi = _describe(case, I, mode=case.imag)
    op_i = _make(I, geom, Bi)
    ki = op_i.dense_kernel()
    assert ki["resident"] and ki["PT"] == case.PT and ki["mode"] == dc.MODES.index(case.imag) and ki["lists"] == case.lists, ki
    assert ceed._lib.load().pa_op_complex_fused(op_r.handle, op_i.handle) == 2  # (2: the dense complex kernel)
    orc_i = Bi.oracle(og)
    n = I.lsize
    xr, xi = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    tdofs = np.nonzero(I.touched)[0]
    lctx = linalg.Context()
    for ess in (np.zeros(0, np.int32), np.sort(rng.choice(tdofs, size=tdofs.size // 7, replace=False)).astype(np.int32)):
        A = linalg.ComplexParOperator(lctx, op_r, op_i, ess, linalg.DIAG_ONE)
        yr, yi = (torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        A.mult(_dev(xr), _dev(xi), yr, yi)
        mr, mi = xr.copy(), xi.copy()
        mr[ess], mi[ess] = 0.0, 0.0
        z = lambda: np.zeros(n)  # noqa: E731
        wr = orc_r.apply_add(mr, z()) - orc_i.apply_add(mi, z())
        wi = orc_i.apply_add(mr, z()) + orc_r.apply_add(mi, z())
        wr[ess], wi[ess] = xr[ess], xi[ess]
        scale = max(np.abs(wr).max(), np.abs(wi).max())
        er, ei = np.abs(yr.cpu().numpy() - wr).max() / scale, np.abs(yi.cpu().numpy() - wi).max() / scale
        print(f"{case.id}: complex apply, {ess.size} essential dofs: {er:.2e} {ei:.2e}")
        assert er < REL and ei < REL
