"""The oracle-side facts tests/test_curl_hex_gpu.py rests on, and its order list against the compiled instantiations of the
discrete curl ND -> RT on hexahedra (palace_amd/csrc/pa_curl_hex.hip).  CPU only."""
import os
import re

import numpy as np
import pytest

from tests import curl_util as cu
from tests import rthex_util as ru
from tests import test_curl_hex_gpu as tg
from tests import transfer_util as tu

CSRC = os.path.join(ru.ROOT, "palace_amd", "csrc")


@pytest.mark.parametrize("p", cu.ORDERS)
def test_element_matrix_is_made_of_1d_blocks(p):
    """rthex.hex_curl_matrix(p) is +- I x Dg x I block by block, to the last bit: what the kernel applies line by line."""
    C, B = cu.matrix(p), cu.block_matrix(p)
    assert C.shape == B.shape == (3 * p * p * (p + 1), 3 * p * (p + 1) ** 2)
    assert np.abs(C - B).max() == 0
    assert (np.count_nonzero(B, axis=1) <= 2 * (p + 1)).all() and np.count_nonzero(B, axis=1).max() == 2 * (p + 1)


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("p", cu.ORDERS)
def test_oracle_equal_copies_and_exact_sequence(kind, p):
    """Every element sharing a Raviart-Thomas dof computes the same curl for it (the device stores one owner copy, the oracle
    the average), and the curl of a discrete gradient vanishes within the bound of the device test."""
    o = cu.oracle(kind, p)
    s = tu.copy_spread(o, ru.vector(o.nc, 3))
    print(f"copies of a shared dof: {s:.2e}")
    assert s < 1e-13
    assert o.inv_mult.min() < 1.0  # (there are shared dofs)
    assert (o.sc < 0).any() and (o.sf < 0).any()
    g = tu.oracle(kind, "grad", p, p).mult(ru.vector(tu.space(kind, "h1", p).ndofs, 11 + p))
    cg = np.abs(o.mult(g)).max()
    print(f"max |C G phi| = {cg:.2e}, bound {cu.exactness_bound(p, g):.2e}")
    assert np.abs(g).max() > 0 and cg <= cu.exactness_bound(p, g)


def test_every_compiled_order_has_a_parity_case():
    """PA_CURL_CASE(P) names the specialised orders; order 5 runs the generic kernel."""
    with open(os.path.join(CSRC, "pa_curl_hex.hip")) as f:
        found = [int(v) for v in re.findall(r"PA_CURL_CASE\(\s*(\d+)\s*\)", f.read())]
    assert sorted(found) == [1, 2, 3, 4] and len(set(found)) == len(found)
    assert tg.CURL_ORDERS == [1, 2, 3, 4, 5] == cu.ORDERS
    assert set(found) <= set(tg.CURL_ORDERS) and 5 in tg.CURL_ORDERS
