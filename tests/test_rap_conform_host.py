"""Host side of the assembled triple product (no GPU): the new entry points load from the built library with their ctypes
signatures, and the true-dof discrete gradient R_nd G_local P_h1 of a constrained pair of lowest-order spaces has the two
properties the auxiliary-space solver relies on -- constants in its kernel, its range in the kernel of the true-dof curl-curl
matrix.  If these failed they would point at the spaces (palace_amd/fem/nchex.py), not at the kernel."""
import ctypes as C

import numpy as np
import pytest

from tests import nc_util as nu
from tests import util


def test_new_symbols_load():
    import __graft_entry__ as ge

    ge.build()
    from palace_amd import lib

    L = lib.load()
    p = C.c_void_p
    sigs = {
        "pa_csr_create": [C.c_int32, C.c_int32, p, p, p, C.c_int, p, p],
        "pa_csr_is_symmetric": [p],
        "pa_csr_rap_conforming": [p, p, p, p, C.c_int, p],
        "pa_csr_rap_conforming_timed": [p, p, p, p, C.c_int, p, p],
        "pa_par_op_parallel_assemble": [p, C.c_int, p],
    }
    for name, argtypes in sigs.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, C.c_int
    # null arguments are reported through the error string, not dereferenced (no device needed to get that far)
    assert L.pa_csr_is_symmetric(None) == -1
    assert L.pa_csr_create(1, 1, None, None, None, 0, None, None) != 0 and b"pa_csr_create" in L.pa_last_error()
    assert L.pa_csr_rap_conforming(None, None, None, None, 0, None) != 0 and b"null argument" in L.pa_last_error()
    assert L.pa_par_op_parallel_assemble(None, 0, None) != 0 and b"null argument" in L.pa_last_error()


@pytest.mark.parametrize("name", ["A", "B"])
def test_true_dof_gradient_properties(name):
    nd, h1 = nu.nc_space(name, "nd", 1), nu.nc_space(name, "h1", 1)
    P_nd, P_h1 = nd.prolongation(), h1.prolongation()
    Gl = nu.local_gradient(h1, nd)
    Gt = (Gl @ P_h1).tocsr()[:nd.n_true]
    # the gradient of a conforming H1 function is a conforming H(curl) function: P_nd G_true = G_local P_h1
    assert abs(P_nd @ Gt - Gl @ P_h1).max() < 1e-14
    assert np.diff(Gt.indptr).max() > 2          # a true edge that ends in a hanging vertex
    assert abs(Gt @ np.ones(h1.n_true)).max() < 1e-14
    K = nu.oracle_local(nd, "hdiv", util.make_ctx("identity")[0], None, 2).assemble_sparse().tocsr()
    Kt = (P_nd.T @ K @ P_nd).tocsr()
    print(f"mesh {name}: max |K_true G_true| {abs(Kt @ Gt).max():.2e} (max |K_true| {abs(Kt).max():.2e})")
    assert abs(Kt @ Gt).max() < 1e-11
