"""The device triple product with conforming prolongations (palace_amd/csrc/pa_rap_conform.hip) against scipy on the three
locally refined meshes of tests/nc_util.py: T = P^T A P of a bilinear form, the injection form R G P of a discrete gradient, the
identity sides, unsorted input with repeated columns, bitwise repeatability, the assembled level operator against the
matrix-free one, and the errors.  Tolerance: the project's parity tolerance, 1e-12 relative to the largest absolute entry -- the
two sides differ only in the summation order over at most a few hundred O(1) products."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import scipy.sparse as sp  # noqa: E402

from oracle import palace_oracle as po  # noqa: E402
from palace_amd import ceed, linalg  # noqa: E402
from tests import nc_util as nu  # noqa: E402
from tests import util  # noqa: E402

TOL = 1e-12
CAP_SMALL, CAP_LARGE = 256, 2048   # products of a row that fit the two LDS forms of the kernel (pa_rap_conform.hip)
ND_CASES = [(m, "nd", p) for m in "ABC" for p in (1, 2)] + [("A", "nd", 3)]
H1_CASES = [(m, "h1", p) for m in "AC" for p in (1, 2)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _relmax(a, b):
    """max |a - b| / max |b| of two scipy matrices of one shape."""
    d = abs(a - b)
    return (d.max() if d.nnz else 0.0) / abs(b).max()


def _ones(m):
    m = m.tocsr()
    return sp.csr_matrix((np.ones(m.indices.size), m.indices, m.indptr), shape=m.shape)


def _sorted_unique(m):
    for r in range(m.shape[0]):
        c = m.indices[m.indptr[r]:m.indptr[r + 1]]
        if c.size > 1 and not (np.diff(c) > 0).all():
            return False
    return True


def _same_pattern(got, structural):
    """`got` as stored (sorted, unique columns) against the pattern of a product of 0 / 1 matrices (no cancellation)."""
    s = structural.tocsr()
    s.sort_indices()
    return np.array_equal(got.indptr, s.indptr) and np.array_equal(got.indices, s.indices)


@pytest.fixture(scope="module")
def ctx():
    return linalg.Context()


_cache = {}


def _case(ctx, name, kind, p):
    """(space, local device operator, its own assembled matrix on the device and as scipy, Conforming, P): made once."""
    key = (name, kind, p)
    if key not in _cache:
        s = nu.nc_space(name, kind, p)
        geom = ceed.GeomFactorData(s.mesh, p + 1)
        if kind == "nd":
            local = ceed.curlcurlmass_operator(geom, s, util.make_ctx("scalar", 2)[1], util.make_ctx("identity")[1])
        else:
            c_mass = po.CoeffCtx(attr_mat=[0], mat_coeff=[np.array([2.08])], dim=1)
            local = ceed.diffusionmass_operator(geom, s, c_mass.pack(), util.make_ctx("identity")[0].pack())
        dcsr = local.full_assemble_device()
        _cache[key] = (s, local, dcsr, dcsr.to_scipy(), linalg.Conforming(ctx, s), s.prolongation(), geom)
    return _cache[key][:6]


def _products(A_loc, P_test, P_trial):
    """Expanded products of every output row: the number the kernel sorts (pattern(P_test)^T pattern(A) rowlen(P_trial))."""
    per_local_row = _ones(A_loc) @ np.diff(P_trial.tocsr().indptr)
    return np.rint(_ones(P_test).T @ per_local_row).astype(np.int64)


@pytest.mark.parametrize("name,kind,p", ND_CASES + H1_CASES)
def test_product_parity(ctx, name, kind, p):
    """T = P^T A_loc P with A_loc the device's own local matrix: values, sorted unique columns, the structural pattern, the
    symmetric flag.  Mesh A at order 3 has rows beyond both LDS forms; every ND case at order >= 2 has rows of all three classes."""
    s, local, dcsr, A_loc, conf, P = _case(ctx, name, kind, p)
    T = linalg.rap_conforming(ctx, dcsr, conf, conf)
    got = T.to_scipy()
    ref = (P.T @ A_loc @ P).tocsr()
    n_prod = _products(A_loc, P, P)
    err = _relmax(got, ref)
    print(f"{name} {kind} p={p}: n_true {s.n_true} nnz {T.nnz} products per row max {n_prod.max()} "
          f"(<= {CAP_SMALL}: {(n_prod <= CAP_SMALL).sum()}, <= {CAP_LARGE}: {((n_prod > CAP_SMALL) & (n_prod <= CAP_LARGE)).sum()}, "
          f"longer: {(n_prod > CAP_LARGE).sum()}) err {err:.2e}")
    assert (T.nrows, T.ncols) == (s.n_true, s.n_true) and got.shape == ref.shape
    assert err < TOL
    assert _sorted_unique(got)
    assert _same_pattern(got, _ones(P).T @ _ones(A_loc) @ _ones(P))
    assert T.symmetric and dcsr.symmetric
    assert (n_prod <= CAP_SMALL).any()
    if (name, kind, p) == ("A", "nd", 3):
        assert (n_prod > CAP_LARGE).any()      # the global-workspace path
    if kind == "nd" and p == 2:
        assert ((n_prod > CAP_SMALL) & (n_prod <= CAP_LARGE)).any()


@pytest.mark.parametrize("name,p", [("A", 1), ("B", 1), ("A", 2)])
def test_injection_form_rectangular(ctx, name, p):
    """The true-dof discrete gradient R_nd G_local P_h1 (first n_true_nd rows of G_local P_h1)."""
    nd, h1 = nu.nc_space(name, "nd", p), nu.nc_space(name, "h1", p)
    Gl = nu.local_gradient(h1, nd)
    G = ceed.DeviceCsr.from_scipy(Gl)
    assert (G.nrows, G.ncols) == Gl.shape and not G.symmetric
    T = linalg.rap_conforming(ctx, G, test=linalg.Conforming(ctx, nd), trial=linalg.Conforming(ctx, h1), injection=True)
    got = T.to_scipy()
    ref = (Gl @ h1.prolongation()).tocsr()[:nd.n_true]
    assert (T.nrows, T.ncols) == (nd.n_true, h1.n_true) and not T.symmetric
    assert _relmax(got, ref) < TOL and _sorted_unique(got)
    assert _same_pattern(got, (_ones(Gl) @ _ones(h1.prolongation())).tocsr()[:nd.n_true])
    if p == 1:
        # a true edge that ends in a hanging vertex: 1, +-1/2 (, +-1/4) instead of the two entries of an incidence matrix
        assert np.diff(got.indptr).max() > 2
        assert abs(got @ np.ones(h1.n_true)).max() < 1e-14


def test_identity_sides(ctx):
    s, local, dcsr, A_loc, conf, P = _case(ctx, "A", "nd", 2)
    both = linalg.rap_conforming(ctx, dcsr).to_scipy()
    srt = A_loc.copy()
    srt.sort_indices()
    assert np.array_equal(both.indptr, srt.indptr) and np.array_equal(both.indices, srt.indices) and np.array_equal(both.data, srt.data)
    right = linalg.rap_conforming(ctx, dcsr, trial=conf)
    assert (right.nrows, right.ncols) == (s.n_local, s.n_true) and not right.symmetric
    assert _relmax(right.to_scipy(), (A_loc @ P).tocsr()) < TOL and _sorted_unique(right.to_scipy())
    left = linalg.rap_conforming(ctx, dcsr, test=conf)
    assert (left.nrows, left.ncols) == (s.n_true, s.n_local) and not left.symmetric
    assert _relmax(left.to_scipy(), (P.T @ A_loc).tocsr()) < TOL and _sorted_unique(left.to_scipy())
    inj = linalg.rap_conforming(ctx, dcsr, test=conf, injection=True)
    assert _relmax(inj.to_scipy(), A_loc[:s.n_true]) < TOL


def test_unsorted_input_with_duplicates(ctx):
    """B with the entries of every row permuted and every third entry split into two halves (a repeated column)."""
    s, local, dcsr, A_loc, conf, P = _case(ctx, "B", "nd", 1)
    rng = np.random.default_rng(17)
    rp, ci, va = [0], [], []
    for r in range(A_loc.shape[0]):
        c = A_loc.indices[A_loc.indptr[r]:A_loc.indptr[r + 1]]
        v = A_loc.data[A_loc.indptr[r]:A_loc.indptr[r + 1]]
        split = np.arange(c.size) % 3 == 0
        c2 = np.concatenate([c, c[split]])
        v2 = np.concatenate([np.where(split, 0.5 * v, v), 0.5 * v[split]])
        perm = rng.permutation(c2.size)
        ci.append(c2[perm]), va.append(v2[perm]), rp.append(rp[-1] + c2.size)
    Bm = sp.csr_matrix((np.concatenate(va), np.concatenate(ci).astype(np.int32), np.array(rp, dtype=np.int32)), shape=A_loc.shape)
    assert Bm.nnz > A_loc.nnz and not Bm.has_sorted_indices
    B = ceed.DeviceCsr.from_scipy(Bm, symmetric=True)
    assert B.nnz == Bm.nnz                      # uploaded as stored
    got = linalg.rap_conforming(ctx, B, conf, conf).to_scipy()
    ref = (P.T @ A_loc @ P).tocsr()
    assert _relmax(got, ref) < TOL and _sorted_unique(got)
    assert _same_pattern(got, _ones(P).T @ _ones(A_loc) @ _ones(P))


@pytest.mark.parametrize("name,kind,p", [("C", "nd", 2), ("A", "nd", 3)])
def test_bit_identical_repeats(ctx, name, kind, p):
    s, local, dcsr, A_loc, conf, P = _case(ctx, name, kind, p)
    a = linalg.rap_conforming(ctx, dcsr, conf, conf).to_scipy()
    b = linalg.rap_conforming(ctx, dcsr, conf, conf).to_scipy()
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)


@pytest.mark.parametrize("name", ["B", "C"])
@pytest.mark.parametrize("policy", [linalg.DIAG_ONE, linalg.DIAG_ZERO])
def test_assembled_level_operator(ctx, name, policy):
    """ParOperator.parallel_assemble() wrapped with the same essential dofs against the three-launch constrained operator.  The
    diagonals are NOT compared with each other: the matrix-free path returns |P|^T diag(A) (rap.cpp:163-175,
    nc_util.ConstrainedParOperatorOracle.diagonal), the assembled one the true diagonal -- it is checked against
    diag(P^T A P) from scipy."""
    s, local, dcsr, A_loc, conf, P = _case(ctx, name, "nd", 1)
    ess = s.ess_dofs()
    A_free = linalg.ParOperator(ctx, local, ess, policy, conforming=conf)
    T = A_free.parallel_assemble()
    assert (T.nrows, T.ncols) == (s.n_true, s.n_true) and T.symmetric
    assert _relmax(T.to_scipy(), (P.T @ A_loc @ P).tocsr()) < TOL
    A_asm = linalg.AssembledParOperator(ctx, T, ess, policy)
    x = np.random.default_rng(3).uniform(-1, 1, s.n_true)
    y_free = A_free.mult(_dev(x), _new(s.n_true)).cpu().numpy()
    y_asm = A_asm.mult(_dev(x), _new(s.n_true)).cpu().numpy()
    assert np.max(np.abs(y_asm - y_free)) < TOL * np.max(np.abs(y_free))
    d = A_asm.assemble_diagonal(_new(s.n_true)).cpu().numpy()
    d_ref = (P.T @ A_loc @ P).diagonal()
    d_ref[ess] = 1.0 if policy == linalg.DIAG_ONE else 0.0
    assert np.max(np.abs(d - d_ref)) < TOL * np.max(np.abs(d_ref))
    # an operator that was created assembled and has no constraint returns its own matrix
    same = linalg.AssembledParOperator(ctx, dcsr, [], policy).parallel_assemble().to_scipy()
    assert np.array_equal(same.indptr, A_loc.indptr) and np.array_equal(same.indices, A_loc.indices) and np.array_equal(same.data, A_loc.data)


def test_errors(ctx):
    s, local, dcsr, A_loc, conf, P = _case(ctx, "A", "nd", 1)
    other = linalg.Conforming(ctx, nu.nc_space("A", "h1", 1))
    with pytest.raises(Exception, match="does not match the rows"):
        linalg.rap_conforming(ctx, dcsr, test=other, trial=conf)
    with pytest.raises(Exception, match="does not match the columns"):
        linalg.rap_conforming(ctx, dcsr, test=conf, trial=other)
    with pytest.raises(Exception, match="column out of range"):
        _bad_upload()
    # an operator with a halo: ranks are out of scope
    ctx1 = linalg.Context()
    ctx1.init_comm_single()
    halo = linalg.Halo(ctx1, [], [], [])
    A = linalg.ParOperator(ctx1, local, [], linalg.DIAG_ONE, n_true=s.n_local, halo=halo)
    with pytest.raises(Exception, match="halo"):
        A.parallel_assemble()


def _bad_upload():
    """pa_csr_create with a column beyond ncols, through the raw entry point (scipy would refuse to build such a matrix)."""
    import ctypes as C

    from palace_amd import lib

    L = lib.load()
    rp, ci, va = np.array([0, 1], dtype=np.int32), np.array([4], dtype=np.int32), np.ones(1)
    L.pa_csr_create.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    h = C.c_void_p()
    lib.check(L.pa_csr_create(1, 4, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), 0, None,
                              C.byref(h)))
