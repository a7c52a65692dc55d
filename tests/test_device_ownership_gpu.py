"""Ownership of device memory (palace_amd/csrc/pa_devbuf.hpp): whatever is created and destroyed through the C interface leaves
pa_device_buffers_live() exactly where it stood -- for every kind of sub-operator, in either order of destroying the geometry
handle and the operators, after a construction that fails on the host, and after fusing an essential list a second time.
The count is the library's own (free-memory readings of a shared card belong to everybody); every assertion is an equality.
Meshes: one hex27 cube split into 2 x 2 x 2, one tetrahedron split into eight."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_cache = {}


def _live():
    from palace_amd import lib

    return lib.device_buffers_live()


def _start():
    gc.collect()  # (objects of earlier tests that were only waiting for the collector go now, not in the middle of this test)
    return _live()


def _destroy(obj):
    """Destroy the library object behind a ceed wrapper now (its __del__ then finds nothing to do)."""
    from palace_amd import ceed, lib

    L = lib.load()
    if isinstance(obj, (ceed.GeomFactorData, ceed.DenseGeomFactorData)):
        L.pa_geom_destroy(obj.handle)
    elif isinstance(obj, ceed.ElementErrorIntegrator):
        L.pa_error_op_destroy(obj.handle)
    elif isinstance(obj, ceed.DeviceCsr):
        L.pa_csr_destroy.restype = None
        L.pa_csr_destroy.argtypes = [C.c_void_p]
        L.pa_csr_destroy(obj.handle)
    else:
        L.pa_op_destroy(obj.handle)
    obj.handle = None


def _hex():
    """(mesh, Nedelec, H1 and Raviart-Thomas spaces of order 2, Nedelec space of order 1) on the 2 x 2 x 2 block."""
    if "hex" not in _cache:
        from palace_amd.fem.fespace import H1HexSpace, NDHexSpace
        from palace_amd.fem.mesh import HexMesh, refine_uniform
        from palace_amd.fem.rthex import RTHexSpace

        n = np.arange(27)
        x = 0.5 * np.stack([n % 3, (n // 3) % 3, n // 9], axis=1).astype(np.float64)
        one = HexMesh(x=x, elem_nodes=n.reshape(1, 27).astype(np.int64), attr=np.ones(1, dtype=np.int32))
        one.check()
        m = refine_uniform(one)
        assert m.ne == 8
        _cache["hex"] = (m, NDHexSpace(m, 2), H1HexSpace(m, 2), RTHexSpace(m, 2), NDHexSpace(m, 1))
    return _cache["hex"]


def _tet():
    """Host data of the eight-tet block: mesh, rule, the curl-oriented Nedelec block and the Raviart-Thomas block (order 2)."""
    if "tet" not in _cache:
        from palace_amd import ceed
        from palace_amd.fem import rt, tet

        m = tet.refine_uniform(tet.TetMesh(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([[0, 1, 2, 3]])))
        assert m.ne == 8
        nd, sp = tet.NDTetSpace(m, 2), rt.RTTetSpace(m, 2)
        pts, wts = tet.tet_quadrature(3)
        nint, ncurl = nd.elem.tables(pts)
        rint, _ = sp.elem.tables(pts)
        assert not nd.diagonal_transform  # (order 2: face dofs in pairs, the tridiagonal curl_orients)
        ndb = ceed.DenseBlock(ceed.FE_HCURL, nd.ndofs, nd.offsets, nint, ncurl, curl_orients=nd.curl_orients)
        rtb = ceed.DenseBlock(ceed.FE_HDIV, sp.ndofs, sp.offsets, rint, None, orients=sp.orients)
        _cache["tet"] = (m, pts, wts, ndb, rtb)
    return _cache["tet"]


def _hex_geom():
    from palace_amd import ceed

    return ceed.GeomFactorData(_hex()[0], 4)


def _tet_geom():
    from palace_amd import ceed

    m, pts, wts, _, _ = _tet()
    return ceed.DenseGeomFactorData(m.elem_nodes, m.nodes, m.attr, m.geometry_grad_table(pts), wts)


def _ctx(kind):
    from tests import util

    return util.make_ctx(kind)[1]


def _vec(n, seed=3):
    import torch

    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, n)).cuda()


def _apply(op):
    import torch

    y = op.mult(_vec(op.width), torch.empty(op.height, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return y


def _prepare_fused_step(op):
    from palace_amd import lib

    avail = C.c_int(0)
    lib.check(lib.load().pa_op_prepare_fused_step(op.handle, C.byref(avail)))
    return avail.value


# ---- one builder per kind: returns (geometry, [objects on it, in creation order]) after one apply of each ----------------------

def _nd_hex_all_forms():
    from palace_amd import ceed

    nd = _hex()[1]
    geom = _hex_geom()
    op = ceed.curlcurl_operator(geom, nd, _ctx("aniso"))  # (packed D of its own; finalized)
    assert op.streams()
    op.set_essential(np.arange(0, nd.ndofs, 7))
    assert _prepare_fused_step(op) == 1  # plain, masked and all: every stream form exists
    _apply(op)
    return geom, [op]


def _h1_hex():
    from palace_amd import ceed

    geom = _hex_geom()
    op = ceed.diffusion_operator(geom, _hex()[2], _ctx("aniso"))
    _apply(op)
    return geom, [op]


def _rt_hex():
    from palace_amd import ceed

    geom = _hex_geom()
    op = ceed.rtmass_operator(geom, _hex()[3], _ctx("aniso"))
    _apply(op)
    return geom, [op]


def _nd_hex_metric_three_holders():
    from palace_amd import ceed

    _, nd, _, _, nd1 = _hex()
    geom = _hex_geom()
    a = ceed.curlcurlmass_operator(geom, nd, _ctx("scalar"), _ctx("identity"))  # isotropic: the metric form of the geometry
    b = ceed.curlcurlmass_operator(geom, nd, _ctx("identity"), _ctx("scalar"))
    c = a.coarsen(geom, nd1)
    for op in (a, b, c):
        _apply(op)
    return geom, [a, b, c]


def _dense_tet():
    from palace_amd import ceed

    ndb = _tet()[3]
    geom = _tet_geom()
    op = ceed.Operator(ndb.lsize, ndb.lsize).add_dense_integrator(geom, ndb, ceed.QF_HDIV_33, _ctx("identity"), ceed.EVAL_CURL).finalize()
    op.set_essential(np.arange(0, ndb.lsize, 5))
    _prepare_fused_step(op)
    _apply(op)
    return geom, [op]


def _two_space_tensor():
    from palace_amd import ceed

    _, nd, _, rt, _ = _hex()
    geom = _hex_geom()
    op = ceed.mixedmass_operator(geom, nd, rt, _ctx("aniso"))
    _apply(op)
    return geom, [op]


def _two_space_dense():
    from palace_amd import ceed

    _, _, _, ndb, rtb = _tet()
    geom = _tet_geom()
    op = ceed.Operator(rtb.lsize, ndb.lsize).add_dense_mixed_integrator(geom, ndb, rtb, ceed.QF_HCURLHDIV_33, _ctx("identity")).finalize()
    _apply(op)
    return geom, [op]


def _error_dense():
    import torch
    from palace_amd import ceed

    _, _, _, ndb, rtb = _tet()
    geom = _tet_geom()
    e = ceed.ElementErrorIntegrator(geom, ndb, rtb, ceed.QF_HCURLHDIV_ERROR_33, np.concatenate([_ctx("identity"), _ctx("identity")]))
    e.apply_add(_vec(ndb.lsize, 4), _vec(rtb.lsize, 5), torch.zeros(e.ne, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return geom, [e]


def _error_tensor():
    import torch
    from palace_amd import ceed

    _, nd, _, rt, _ = _hex()
    geom = _hex_geom()
    e = ceed.HexElementErrorIntegrator(geom, nd, rt, ceed.QF_HCURLHDIV_ERROR_33, np.concatenate([_ctx("aniso"), _ctx("identity")]))
    e.apply_add(_vec(nd.ndofs, 4), _vec(rt.ndofs, 5), torch.zeros(e.ne, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return geom, [e]


def _assembled_csr():
    from palace_amd import ceed

    geom = _hex_geom()
    op = ceed.diffusion_operator(geom, _hex()[2], _ctx("aniso"))
    return geom, [op, op.full_assemble_device(), op.full_assemble_device(skip_zeros=True)]


KINDS = {"nd_hex_all_forms": _nd_hex_all_forms, "h1_hex": _h1_hex, "rt_hex": _rt_hex,
         "nd_hex_metric_three_holders": _nd_hex_metric_three_holders, "dense_tet": _dense_tet,
         "two_space_tensor": _two_space_tensor, "two_space_dense": _two_space_dense, "error_dense": _error_dense,
         "error_tensor": _error_tensor, "assembled_csr": _assembled_csr}


@pytest.mark.parametrize("geom_first", [False, True], ids=["operators_first", "geometry_first"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_round_trip(kind, geom_first):
    start = _start()
    geom, objs = KINDS[kind]()
    assert _live() > start
    if geom_first:
        _destroy(geom)  # (the operators keep the geometry data alive)
        assert _live() > start
    for o in reversed(objs):
        _destroy(o)
    if not geom_first:
        assert _live() > start  # (the geometry data is still there)
        _destroy(geom)
    assert _live() == start


def _add_sub_raw(op, geom, space, qf, ctx_ptr, ctx_size, ops):
    from palace_amd import ceed, lib

    r, k1 = ceed._restriction_desc(space)
    b, k2 = ceed._basis_desc(space, geom.q1d)
    return lib.load().pa_op_add_sub(op.handle, geom.handle, C.byref(r), C.byref(b), C.c_int32(qf), ctx_ptr, C.c_size_t(ctx_size),
                                    C.c_uint32(ops), C.c_uint32(ops))


@pytest.mark.parametrize("case", ["short_context", "null_context"])
def test_failed_hex_construction_releases_everything(case):
    from palace_amd import ceed, lib

    nd = _hex()[1]
    start = _start()
    geom = _hex_geom()
    op = ceed.Operator(nd.ndofs, nd.ndofs)
    short = np.zeros(1)  # 8 bytes
    rc = (_add_sub_raw(op, geom, nd, ceed.QF_HDIV_33, short.ctypes.data_as(C.c_void_p), 8, ceed.EVAL_CURL) if case == "short_context"
          else _add_sub_raw(op, geom, nd, ceed.QF_HDIV_33, None, 24, ceed.EVAL_CURL))
    assert rc != 0
    assert lib.last_error() != ""
    _destroy(op)
    _destroy(geom)
    assert _live() == start


@pytest.mark.parametrize("case", ["offset_out_of_range", "bad_curl_orientation"])
def test_failed_dense_construction_releases_everything(case):
    from palace_amd import ceed, lib

    ndb = _tet()[3]
    off, cor = ndb.offsets.copy(), ndb.curl_orients.copy()
    if case == "offset_out_of_range":
        off[ndb.ne - 1, ndb.P - 1] = ndb.lsize
    else:
        cor[ndb.ne - 1, ndb.P - 1, 1] = 2
    bad = ceed.DenseBlock(ceed.FE_HCURL, ndb.lsize, off, ndb.interp, ndb.deriv, curl_orients=cor)
    start = _start()
    geom = _tet_geom()
    op = ceed.Operator(ndb.lsize, ndb.lsize)
    r, b = bad.descs()
    ctx = np.ascontiguousarray(_ctx("identity"))
    rc = lib.load().pa_op_add_sub_dense(op.handle, geom.handle, C.byref(r), C.byref(b), C.c_int32(ceed.QF_HDIV_33),
                                        ctx.ctypes.data_as(C.c_void_p), C.c_size_t(ctx.nbytes), C.c_uint32(ceed.EVAL_CURL),
                                        C.c_uint32(ceed.EVAL_CURL))
    assert rc != 0
    assert lib.last_error() != ""
    _destroy(op)
    _destroy(geom)
    assert _live() == start


def test_fusing_again_keeps_the_count():
    from palace_amd import ceed

    nd = _hex()[1]
    start = _start()
    geom = _hex_geom()
    op = ceed.curlcurl_operator(geom, nd, _ctx("aniso"))
    ess = np.arange(0, nd.ndofs, 7)
    op.set_essential(ess)
    fused = _live()
    op.set_essential(ess)
    assert _live() == fused
    assert _prepare_fused_step(op) == 1
    prepared = _live()
    assert _prepare_fused_step(op) == 1
    assert _live() == prepared
    op.set_essential(ess)  # (drops the `all` form: built again by the next prepare)
    assert _prepare_fused_step(op) == 1
    assert _live() == prepared
    _destroy(op)
    _destroy(geom)
    assert _live() == start
