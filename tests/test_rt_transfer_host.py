"""The oracle-side facts the Raviart-Thomas p-prolongation (palace_amd/csrc/pa_prolong_rt_hex.hip) and its tests rest on, for all
ten pairs 1 <= pc < pf <= 5: the element matrix of tests/rt_transfer_util.py is an exact embedding (values and divergences at
quadrature points), commutes with the discrete curl, gives equal copies of every shared fine dof on the two rotated meshes of
tests/rthex_util.py (so the device may store one owner copy), and P^T M_f P is the coarse mass assembled on the fine rule (so a
p-multigrid hierarchy assembles every level on its own space).  Keeps the pair list of tests/test_rt_transfer_gpu.py in step
with the compiled one.  CPU only."""
import os
import re

import numpy as np
import pytest

from oracle import palace_oracle as po
from tests import curl_util as cu
from tests import rt_transfer_util as rtu
from tests import rthex_util as ru
from tests import test_rt_transfer_gpu as tg
from tests import transfer_util as tu

TOL = 1e-13  # every fact below; measured <= 9.9e-15 (the divergence at (1, 5))


def _compiled_pairs():
    """(specialised, generic) pairs of PA_RT_PROLONG_LIST."""
    with open(os.path.join(ru.ROOT, "palace_amd", "csrc", "pa_prolong_rt_hex.hip")) as f:
        body = re.search(r"#define PA_RT_PROLONG_LIST\(S, G\)(.*?)\n", f.read()).group(1)
    pairs = lambda tag: [(int(a), int(b)) for a, b in re.findall(tag + r"\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]  # noqa: E731
    return pairs("S"), pairs("G")


def test_every_compiled_pair_has_a_parity_case():
    spec, gen = _compiled_pairs()
    assert len(spec) == 6 and len(gen) == 4 and len(set(spec + gen)) == 10
    assert all(pf <= 4 for _, pf in spec) and all(pf == 5 for _, pf in gen)  # Ic / Io by value hold pf <= 4
    assert sorted(spec + gen) == sorted(tg.PAIRS) == sorted(rtu.PAIRS) and len(set(tg.PAIRS)) == len(tg.PAIRS)
    assert sorted(tg.GALERKIN_PAIRS) == sorted(spec)


@pytest.mark.parametrize("pc,pf", rtu.PAIRS)
def test_exact_embedding(pc, pf):
    """Values (absolute) and divergences (max |delta| / max |div|) of the prolonged function equal the coarse function's on
    the (pf + 1)-point rule."""
    P = rtu.matrix(pc, pf)
    vc, dc = ru.tables(pc, pf + 1)
    vf, df = ru.tables(pf, pf + 1)
    e_v = np.abs(vf @ P - vc).max()
    e_d = np.abs(df @ P - dc).max() / np.abs(dc).max()
    print(f"values {e_v:.2e} divergences {e_d:.2e}")
    assert e_v < TOL
    assert e_d < TOL


@pytest.mark.parametrize("pc,pf", rtu.PAIRS)
def test_commutes_with_the_curl_on_the_element(pc, pf):
    """C_f P_nd = P_rt C_c."""
    a = cu.matrix(pf) @ po.nd_hex_interp_lex(pc, pf)
    b = rtu.matrix(pc, pf) @ cu.matrix(pc)
    err = np.abs(a - b).max() / np.abs(a).max()
    print(f"commuting diagram {err:.2e}")
    assert np.abs(a).max() > 0.0 and err < TOL


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("pc,pf", rtu.PAIRS)
def test_equal_copies_and_negative_signs(kind, pc, pf):
    """Every element sharing a fine dof computes the same value for it, and both levels carry negative orientation signs."""
    o = rtu.oracle(kind, pc, pf)
    s = tu.copy_spread(o, ru.vector(o.nc, 3))
    print(f"copies of a shared dof: {s:.2e}")
    assert s < TOL
    assert o.inv_mult.min() < 1.0  # (there are shared dofs)
    c, f = rtu.spaces(kind, pc, pf)
    assert (c.elem_sign_lex < 0).any() and (f.elem_sign_lex < 0).any()
    neg = ((o.sc[:, None, :] * o.sf[:, :, None] < 0) & (o.M[None] != 0.0)).sum() / (o.dc.shape[0] * np.count_nonzero(o.M))
    assert 0.1 < neg < 0.6, neg  # (a share of the element entries enters with a negative sign)


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("pc,pf", rtu.PAIRS)
def test_galerkin_operator_is_the_coarse_mass_on_the_fine_rule(kind, pc, pf):
    """P^T M_f P x = M_c x, M_c the mass of order pc on the rule of order pf (two materials, anisotropic coefficient)."""
    o = rtu.oracle(kind, pc, pf)
    Mf, Mc = rtu.mass_oracle(kind, pf, pf + 1), rtu.mass_oracle(kind, pc, pf + 1)
    x = ru.vector(o.nc, 11 + 10 * pc + pf)
    a = o.mult_transpose(Mf.apply_add(o.mult(x), np.zeros(o.nf)))
    b = Mc.apply_add(x, np.zeros(o.nc))
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"Galerkin {err:.2e}")
    assert err < TOL


@pytest.mark.parametrize("kind,p", [("ogrid15", 2), ("ogrid15", 3), ("cyl80", 3), ("ogrid15", 4)])
def test_oracle_multigrid_needs_fewer_iterations_than_jacobi(kind, p):
    """PCG to 1e-12 on the unit-coefficient mass: the p-multigrid cycle over levels 1 .. p (4th-kind Chebyshev order 2, one pre
    and one post step, exact coarse solve) against Jacobi (measured 7 against 22 - 25)."""
    it_j, it_mg = rtu.oracle_counts(kind, p)
    print(f"{kind} p = {p}: Jacobi {it_j}, p-multigrid {it_mg}")
    assert 0 < it_mg < it_j
