"""Both parts of a complex field per pass on tensor-product hexahedra (palace_amd/csrc/pa_mixed_hex2.hip, pa_rt_hex2.hip behind
pa_op_mult2 / pa_op_mult2_essential_diag / pa_error_op_apply_add2): the two-space mass, the element error integrator and the
Raviart-Thomas operators with two right-hand sides against the oracle, against the one-part kernels (to the bit where the
arithmetic is the same) and as the estimator procedure for a complex field.  Meshes, materials and helpers are those of
tests/test_mixed_hex_gpu.py and tests/test_rt_hex_gpu.py (tests/rthex_util.py: cyl80 gives whole blocks at every rule,
ogrid15 a partial wave at every rule; every element rotated, negative orientation signs)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import rthex_util as ru
from tests import test_mixed_hex_gpu as mh
from tests import test_rt_hex_gpu as rh
from tests import util

pytestmark = pytest.mark.gpu

PQ = mh.PQ
REL = 1e-12  # the project's operator-level tolerance
_cache = {}


def compiled_pairs(macro, source):
    """The (p, q1d) pairs of a PA_*2_CASE list, parsed from the source as tests/test_hex_instantiations.py parses its lists."""
    with open(os.path.join(ru.ROOT, "palace_amd", "csrc", source)) as f:
        found = re.findall(macro + r"\(\s*(\d+)\s*,\s*(\d+)\s*\)", f.read())
    return [(int(p), int(q)) for p, q in found]


MIXED2 = compiled_pairs("PA_MIXED2_CASE", "pa_mixed_hex2.hip")
ERROR2 = compiled_pairs("PA_ERROR2_CASE", "pa_mixed_hex2.hip")
RT2 = compiled_pairs("PA_RT2_CASE", "pa_rt_hex2.hip")


def _mult2(op, x0, x1):
    import torch

    y0 = torch.full((op.height,), 7.0, dtype=torch.float64, device="cuda")  # Mult overwrites
    y1 = torch.full((op.height,), -3.0, dtype=torch.float64, device="cuda")
    op.mult2(mh._dev(x0), mh._dev(x1), y0, y1)
    return y0.cpu().numpy(), y1.cpu().numpy()


def _mass_reference_imag(kind, p, q1d, nd_trial):
    """(x_i, (v, C x_i) of the oracle) next to the cached real-part reference of tests/test_mixed_hex_gpu.py."""
    key = ("mass_i", kind, p, q1d, nd_trial)
    if key not in _cache:
        (tr, tro), (te, teo) = mh._sides(kind, p, q1d, nd_trial)
        x = ru.vector(tr.ndofs, 200 * p + q1d + int(nd_trial))
        qfo = po.QF_HCURLHDIV if nd_trial else po.QF_HDIVHCURL
        ref = po.MixedSpaceOracle(tro, teo, mh._ogeom(kind, q1d), qfo, ru.mass_ctx("nonsym")).apply_add(x, np.zeros(te.ndofs))
        ref.setflags(write=False)
        _cache[key] = (x, ref)
    return _cache[key]


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("nd_trial", [True, False], ids=["hcurlhdiv", "hdivhcurl"])
@pytest.mark.parametrize("p,q1d", PQ)
def test_mixed_mass_two_parts(p, q1d, nd_trial, kind):
    """mult2 against the oracle on each part, against mult on each part to the bit, and against A^T of the other QFunction's
    operator with the transposed material (mult_transpose) on both parts."""
    op = mh._mass_operator(kind, p, q1d, nd_trial)
    assert op.two_rhs() == ((p, q1d) in MIXED2)
    (xr, ref_r), (xi, ref_i) = mh._mass_reference(kind, p, q1d, nd_trial, "nonsym"), _mass_reference_imag(kind, p, q1d, nd_trial)
    yr, yi = _mult2(op, xr, xi)
    er, ei = mh._relerr(yr, ref_r), mh._relerr(yi, ref_i)
    print(f"mult2 against the oracle {er:.2e} {ei:.2e}")
    assert er < REL and ei < REL
    dr, di = np.abs(yr - mh._mult(op, xr)), np.abs(yi - mh._mult(op, xi))
    print(f"mult2 against mult: {np.count_nonzero(dr)} and {np.count_nonzero(di)} entries differ, by at most {max(dr.max(), di.max()):.2e}")
    assert np.array_equal(yr, mh._mult(op, xr)) and np.array_equal(yi, mh._mult(op, xi))
    # the other QFunction's operator with every material matrix transposed is A^T: its transposed apply maps like A itself
    other = mh._mass_operator(kind, p, q1d, not nd_trial, "nonsym_t")
    assert other.height == op.width and other.width == op.height
    zr, zi = ru.vector(op.width, 17), ru.vector(op.width, 18)
    yr, yi = _mult2(op, zr, zi)
    er, ei = mh._relerr(yr, mh._mult(other, zr, transpose=True)), mh._relerr(yi, mh._mult(other, zi, transpose=True))
    print(f"mult2 against the transposed apply {er:.2e} {ei:.2e}")
    assert er < 1e-13 and ei < 1e-13


def _error_integrator(kind, p, q1d, nd_first):
    from palace_amd import ceed

    (s1, _), (s2, _) = mh._sides(kind, p, q1d, nd_first)
    _, b_an = util.make_ctx("aniso", 2)
    _, b_ns = util.make_ctx("nonsym", 2)
    qf = ceed.QF_HCURLHDIV_ERROR_33 if nd_first else ceed.QF_HDIVHCURL_ERROR_33
    return ceed.HexElementErrorIntegrator(mh._geom(kind, q1d), s1, s2, qf, np.concatenate([b_an, b_ns]))


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("nd_first", [True, False], ids=["hcurlhdiv_error", "hdivhcurl_error"])
@pytest.mark.parametrize("p,q1d", PQ)
def test_element_error_two_parts(p, q1d, nd_first, kind):
    """apply_add2 into a non-zero vector: against the oracle's error_add of the real part plus that of the imaginary part,
    against two apply_add calls, identical bits on a second call; the estimates are in the caller's element order."""
    geom = mh._geom(kind, q1d)
    if kind == "cyl80":
        assert not np.array_equal(mh._element_order(geom), np.arange(geom.mesh.ne))
    (s1, o1), (s2, o2) = mh._sides(kind, p, q1d, nd_first)
    c_an, _ = util.make_ctx("aniso", 2)
    c_ns, _ = util.make_ctx("nonsym", 2)
    qfo = po.QF_HCURLHDIV_ERROR if nd_first else po.QF_HDIVHCURL_ERROR
    integ = _error_integrator(kind, p, q1d, nd_first)
    assert integ.two_parts() == ((p, q1d) in ERROR2)
    rng = np.random.default_rng(10 * p + q1d)
    u1r, u2r = rng.uniform(-1, 1, s1.ndofs), rng.uniform(-1, 1, s2.ndofs)
    u1i, u2i = rng.uniform(-1, 1, s1.ndofs), rng.uniform(-1, 1, s2.ndofs)
    e0 = rng.uniform(0, 1, integ.ne)
    orc = po.MixedSpaceOracle(o1, o2, mh._ogeom(kind, q1d), qfo, c_an, c_ns)
    ref = orc.error_add(u1i, u2i, orc.error_add(u1r, u2r, e0.copy()))
    dev = [mh._dev(v) for v in (u1r, u2r, u1i, u2i)]
    est = integ.apply_add2(*dev, mh._dev(e0.copy())).cpu().numpy()
    e = np.abs(est - ref).max() / ref.max()
    print(f"against the oracle {e:.2e}")
    assert e < REL and (ref - e0).min() > 0
    two = mh._dev(e0.copy())
    integ.apply_add(dev[0], dev[1], two)
    integ.apply_add(dev[2], dev[3], two)
    e = np.abs(est - two.cpu().numpy()).max() / ref.max()
    print(f"against two passes {e:.2e}")
    assert e < 1e-13
    assert np.array_equal(est, integ.apply_add2(*dev, mh._dev(e0.copy())).cpu().numpy())


def test_dense_error_operator_two_parts():
    """The dense-table operator of pa_error_op_create through the same entry point: its two passes."""
    from palace_amd import ceed

    p, kind = 1, "cyl80"
    dgeom, ndb, rtb = mh._dense_setup(p)
    nd, sp = mh._spaces(kind, p)
    _, b_an = util.make_ctx("aniso", 2)
    _, b_ns = util.make_ctx("nonsym", 2)
    integ = ceed.ElementErrorIntegrator(dgeom, ndb, rtb, ceed.QF_HCURLHDIV_ERROR_33, np.concatenate([b_an, b_ns]))
    assert not integ.two_parts()
    dev = [mh._dev(ru.vector(n, s)) for n, s in ((nd.ndofs, 4), (sp.ndofs, 6), (nd.ndofs, 7), (sp.ndofs, 8))]
    e0 = np.random.default_rng(3).uniform(0, 1, integ.ne)
    est = integ.apply_add2(*dev, mh._dev(e0.copy())).cpu().numpy()
    two = mh._dev(e0.copy())
    integ.apply_add(dev[0], dev[1], two)
    integ.apply_add(dev[2], dev[3], two)
    assert np.array_equal(est, two.cpu().numpy()) and (est - e0).min() > 0


def _essential(L, op, x, policy):
    import torch

    from palace_amd import lib

    y = torch.full((x.numel(),), 7.0, dtype=torch.float64, device="cuda")
    handled = C.c_int(-1)
    lib.check(L.pa_op_mult_essential_diag(op.handle, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_int(policy), None,
                                          C.byref(handled)))
    return y.cpu().numpy(), handled.value


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("form", rh.FORMS)
@pytest.mark.parametrize("p,q1d", RT2)
def test_rt_two_rhs(p, q1d, form, kind):
    """Packed D: mult2 equals mult to the bit, and pa_op_mult2_essential_diag the one-vector essential apply on the boundary
    dofs, under both diagonal policies."""
    import torch

    from palace_amd import lib

    op = rh._operator(kind, p, q1d, form)
    assert op.two_rhs()
    n = ru.space(kind, p).ndofs
    x0, x1 = ru.vector(n, 1), ru.vector(n, 2)
    y0, y1 = _mult2(op, x0, x1)
    d0, d1 = np.abs(y0 - rh._mult(op, x0)), np.abs(y1 - rh._mult(op, x1))
    print(f"mult2 against mult: {np.count_nonzero(d0)} and {np.count_nonzero(d1)} entries differ, by at most {max(d0.max(), d1.max()):.2e}")
    assert np.array_equal(y0, rh._mult(op, x0)) and np.array_equal(y1, rh._mult(op, x1))
    xo, ref = ru.oracle_mult(kind, p, q1d, form)
    assert rh._relerr(_mult2(op, xo, x1)[0], ref) < REL
    L = lib.load()
    op.set_essential(ru.boundary_dofs(kind, p))
    d0, d1 = mh._dev(x0), mh._dev(x1)
    for policy in (1, 0):
        r0, h0 = _essential(L, op, d0, policy)
        r1, _ = _essential(L, op, d1, policy)
        z0 = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        z1 = torch.full((n,), -3.0, dtype=torch.float64, device="cuda")
        handled = C.c_int(-1)
        lib.check(L.pa_op_mult2_essential_diag(op.handle, C.c_void_p(d0.data_ptr()), C.c_void_p(d1.data_ptr()),
                                               C.c_void_p(z0.data_ptr()), C.c_void_p(z1.data_ptr()), C.c_int(policy), None,
                                               C.byref(handled)))
        assert handled.value == h0
        if not h0:  # the caller fixes the essential rows: compare the others
            keep = np.setdiff1d(np.arange(n), ru.boundary_dofs(kind, p))
            assert np.array_equal(z0.cpu().numpy()[keep], r0[keep]) and np.array_equal(z1.cpu().numpy()[keep], r1[keep])
        else:
            assert np.array_equal(z0.cpu().numpy(), r0) and np.array_equal(z1.cpu().numpy(), r1)


def test_rt_matrix_free_keeps_two_applies(monkeypatch):
    """A matrix-free operator (non-symmetric material) has no two-vector kernel and still returns both results."""
    monkeypatch.setenv("PALACE_AMD_QDATA", "0")
    kind, p, q1d = "ogrid15", 2, 3
    op = rh._operator(kind, p, q1d, "mass", mass="nonsym")
    assert not op.two_rhs()
    n = ru.space(kind, p).ndofs
    x0, x1 = ru.vector(n, 1), ru.vector(n, 2)
    y0, y1 = _mult2(op, x0, x1)
    assert np.array_equal(y0, rh._mult(op, x0)) and np.array_equal(y1, rh._mult(op, x1))
    _, ref = ru.oracle_mult(kind, p, q1d, "mass", "nonsym", x=x0)
    assert rh._relerr(y0, ref) < REL


_CHILD = """
import ctypes as C
import numpy as np
import torch
from palace_amd import lib
from tests import rthex_util as ru, test_mixed_hex_gpu as mh, test_rt_hex_gpu as rh, test_two_part_hex_gpu as tp
kind, p, q1d = "ogrid15", 2, 3
assert (p, q1d) in tp.MIXED2 and (p, q1d) in tp.ERROR2 and (p, q1d) in tp.RT2
op = mh._mass_operator(kind, p, q1d, True)
rt = rh._operator(kind, p, q1d, "mass")
integ = tp._error_integrator(kind, p, q1d, True)
assert not op.two_rhs() and not rt.two_rhs() and not integ.two_parts()
x0, x1 = ru.vector(op.width, 1), ru.vector(op.width, 2)
y0, y1 = tp._mult2(op, x0, x1)
assert np.array_equal(y0, mh._mult(op, x0)) and np.array_equal(y1, mh._mult(op, x1))
# the Raviart-Thomas operator: mult2, then the essential form, whose rows the caller or the gather fixes
n = rt.height
r0, r1 = ru.vector(n, 3), ru.vector(n, 4)
y0, y1 = tp._mult2(rt, r0, r1)
assert np.array_equal(y0, rh._mult(rt, r0)) and np.array_equal(y1, rh._mult(rt, r1))
L = lib.load()
ess = ru.boundary_dofs(kind, p)
rt.set_essential(ess)
keep = np.setdiff1d(np.arange(n), ess)
d0, d1 = mh._dev(r0), mh._dev(r1)
for policy in (1, 0):
    e0, h0 = tp._essential(L, rt, d0, policy)
    e1, _ = tp._essential(L, rt, d1, policy)
    z0, z1 = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), torch.full((n,), -3.0, dtype=torch.float64, device="cuda")
    handled = C.c_int(-1)
    lib.check(L.pa_op_mult2_essential_diag(rt.handle, C.c_void_p(d0.data_ptr()), C.c_void_p(d1.data_ptr()), C.c_void_p(z0.data_ptr()),
                                           C.c_void_p(z1.data_ptr()), C.c_int(policy), None, C.byref(handled)))
    assert handled.value == 0  # two applies: the caller fixes the essential rows
    assert np.array_equal(z0.cpu().numpy()[keep], e0[keep]) and np.array_equal(z1.cpu().numpy()[keep], e1[keep])
# the error integrator: apply_add2 is the two passes
(s1, _), (s2, _) = mh._sides(kind, p, q1d, True)
dev = [mh._dev(ru.vector(m, s)) for m, s in ((s1.ndofs, 5), (s2.ndofs, 6), (s1.ndofs, 7), (s2.ndofs, 8))]
start = np.random.default_rng(3).uniform(0, 1, integ.ne)
est = integ.apply_add2(*dev, mh._dev(start.copy())).cpu().numpy()
two = mh._dev(start.copy())
integ.apply_add(dev[0], dev[1], two)
integ.apply_add(dev[2], dev[3], two)
assert np.array_equal(est, two.cpu().numpy()) and (est - start).min() > 0
print("CHILD OK")
"""


def test_switch_forces_two_passes():
    """PALACE_AMD_TWO_PART=0 in a child process: every capability query answers 0; mult2 on the two-space and the Raviart-Thomas
    operator, pa_op_mult2_essential_diag and apply_add2 return what two one-part passes return."""
    env = dict(os.environ, PALACE_AMD_TWO_PART="0")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ru.ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout + r.stderr


def complex_device_estimate(mesh, p, direction, field_r, field_i, mats=None):
    """The estimator procedure for a complex field through the Python mirror at order p with p + 1 points per direction: flux
    through mult2, ComplexParCg + Jacobi on the smooth space's mass (rel. tol 1e-13), apply_add2.  Returns (estimates,
    (smooth flux real, imaginary), PCG iterations)."""
    import torch

    from palace_amd import ceed, linalg
    from palace_amd.fem import rthex
    from palace_amd.fem.fespace import NDHexSpace

    nd, sp = NDHexSpace(mesh, p), rthex.RTHexSpace(mesh, p)
    rhs_sp, smooth = (nd, sp) if direction == "grad" else (sp, nd)
    c_mat, c_sq, c_isq = mh.estimator_materials(mats)
    geom = ceed.GeomFactorData(mesh, p + 1)
    ctx = linalg.Context()
    flux = ceed.mixedmass_operator(geom, rhs_sp, smooth, c_mat.pack())
    mass = (ceed.rtmass_operator if direction == "grad" else ceed.ndmass_operator)(geom, smooth, po.CoeffCtx().pack())
    M = linalg.ComplexParOperator(ctx, mass, None)
    Mr = linalg.ParOperator(ctx, mass, np.zeros(0, np.int32), linalg.DIAG_ONE)
    cg = linalg.ComplexParCg(ctx, M, linalg.jacobi(ctx, Mr), rel_tol=1e-13, max_it=1000)
    qf = ceed.QF_HCURLHDIV_ERROR_33 if direction == "grad" else ceed.QF_HDIVHCURL_ERROR_33
    integ = ceed.HexElementErrorIntegrator(geom, rhs_sp, smooth, qf, np.concatenate([c_sq.pack(), c_isq.pack()]))
    Fr, Fi = mh._dev(field_r), mh._dev(field_i)
    br = torch.empty(smooth.ndofs, dtype=torch.float64, device="cuda")
    bi = torch.empty_like(br)
    flux.mult2(Fr, Fi, br, bi)
    Dr, Di = torch.zeros_like(br), torch.zeros_like(br)
    cg.mult(br, bi, Dr, Di)
    assert cg.stats()["converged"]
    est = integ.apply_add2(Fr, Dr, Fi, Di, torch.zeros(integ.ne, dtype=torch.float64, device="cuda"))
    return est.cpu().numpy(), (Dr.cpu().numpy(), Di.cpu().numpy()), cg.stats()["iterations"]


@pytest.mark.parametrize("direction", ["grad", "curl"])
@pytest.mark.parametrize("p", [3, 4])
def test_complex_flux_error_estimate(p, direction):
    """ComputeErrorEstimates for a ComplexVector (errorestimator.cpp:189-268) with the library's pieces, against the oracle
    procedure of tests/test_mixed_hex_gpu.py::_estimate run on each part with a dense solve."""
    kind, q1d = "ogrid15", p + 1
    (s1, o1), (s2, o2) = mh._sides(kind, p, q1d, direction == "grad")
    Er, Ei = ru.vector(s1.ndofs, 3), ru.vector(s1.ndofs, 31)
    est, (Dr, Di), _ = complex_device_estimate(mh._mesh(kind), p, direction, Er, Ei)
    c_eps, c_sq, c_isq = mh.estimator_materials()
    og = mh._ogeom(kind, q1d)
    Mo = po.CeedOperatorOracle(o2.lsize, o2.off, o2.sgn < 0, o2.interp, o2.interp, og,
                               po.QF_HDIV if direction == "grad" else po.QF_HCURL, po.CoeffCtx()).assemble_sparse().toarray()
    qfo, qfe = ((po.QF_HCURLHDIV, po.QF_HCURLHDIV_ERROR) if direction == "grad" else (po.QF_HDIVHCURL, po.QF_HDIVHCURL_ERROR))
    flux_o, err_o = po.MixedSpaceOracle(o1, o2, og, qfo, c_eps), po.MixedSpaceOracle(o1, o2, og, qfe, c_sq, c_isq)
    est_o = np.zeros(o1.NE)
    for part, D in ((Er, Dr), (Ei, Di)):
        D_o = np.linalg.solve(Mo, flux_o.apply_add(part, np.zeros(s2.ndofs)))
        eD = mh._relerr(D, D_o)
        print(f"smooth flux {eD:.2e}")
        assert eD < 1e-9
        est_o = err_o.error_add(part, D_o, est_o)
    ee = np.abs(est - est_o).max() / est_o.max()
    print(f"estimates {ee:.2e}")
    assert ee < 1e-9 and est_o.min() > 0
