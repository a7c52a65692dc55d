"""Keeps the case lists of the GPU tests in step with the compiled instantiations: every PA_INTERP_CASE(K, PC, PF) of
palace_amd/csrc/pa_interp.hip and every (p, q1d) pair of PA_HEX_PQ_LIST (pa_hex_core.hpp) must have a parity case.  And the
oracle-side facts tests/test_hex_transfer_gpu.py rests on, on the two rotated meshes of tests/rthex_util.py.  CPU only."""
import os
import re

import pytest

from tests import rthex_util as ru
from tests import test_hex_transfer_gpu as tg
from tests import transfer_util as tu

CSRC = os.path.join(ru.ROOT, "palace_amd", "csrc")
PAIRS = [(pc, pf) for pf in range(2, 6) for pc in range(1, pf)]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _compiled_transfers():
    """{kind: {(pc, pf)}} of the specialised instantiations (KIND 0: ND, 1: gradient, 2: H1)."""
    found = re.findall(r"PA_INTERP_CASE\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", _read("pa_interp.hip"))
    out = {"nd": set(), "grad": set(), "h1": set()}
    for k, pc, pf in found:
        out[("nd", "grad", "h1")[int(k)]].add((int(pc), int(pf)))
    return out, len(found)


def _compiled_pq():
    body = re.search(r"#define PA_HEX_PQ_LIST\(X, \.\.\.\)(.*?)\n#define", _read("pa_hex_core.hpp"), re.S).group(1)
    return [(int(p), int(q)) for p, q in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,", body)]


def test_every_compiled_transfer_has_a_parity_case():
    compiled, n = _compiled_transfers()
    assert n == 16 == sum(len(v) for v in compiled.values())  # (the expression found the list, no case twice)
    assert compiled["nd"] <= set(tg.ND_PAIRS) and compiled["h1"] <= set(tg.H1_PAIRS)
    assert compiled["grad"] <= {(p, p) for p in tg.GRAD_ORDERS}
    # the generic kernel in all three kinds: an order-5 case each (nothing is specialised there: Ic_s / Io_s hold pf <= 4)
    assert not any(pf == 5 for v in compiled.values() for _, pf in v)
    assert any(pf == 5 for _, pf in tg.ND_PAIRS) and any(pf == 5 for _, pf in tg.H1_PAIRS) and 5 in tg.GRAD_ORDERS
    assert set(tg.ND_PAIRS) == set(PAIRS) == set(tg.H1_PAIRS) and sorted(tg.GRAD_ORDERS) == [1, 2, 3, 4, 5]
    for lst in (tg.ND_PAIRS, tg.H1_PAIRS, tg.GRAD_ORDERS):
        assert len(set(lst)) == len(lst)


def test_every_compiled_rule_pair_has_a_parity_case():
    from tests import test_h1_gpu, test_mixed_hex_gpu, test_rt_hex_gpu

    pq = _compiled_pq()
    assert len(pq) == 10 == len(set(pq))
    for mod in (test_h1_gpu, test_rt_hex_gpu, test_mixed_hex_gpu):
        assert set(pq) <= set(mod.PQ), (mod.__name__, sorted(set(pq) - set(mod.PQ)))
        assert len(set(mod.PQ)) == len(mod.PQ)


@pytest.mark.parametrize("kind", ru.MESHES)
@pytest.mark.parametrize("pc,pf", PAIRS)
def test_oracle_commuting_diagram_and_equal_copies(kind, pc, pf):
    """G_f P_h1 phi = P_nd G_c phi through the oracle alone, and every element sharing a fine dof computes the same value for
    it: the device stores one owner copy, the oracle the average of all (spread measured: 4e-16)."""
    P_h1, P_nd = tu.oracle(kind, "h1", pc, pf), tu.oracle(kind, "nd", pc, pf)
    G_c, G_f = tu.oracle(kind, "grad", pc, pc), tu.oracle(kind, "grad", pf, pf)
    phi = ru.vector(P_h1.nc, 7 + 10 * pc + pf)
    a, b = G_f.mult(P_h1.mult(phi)), P_nd.mult(G_c.mult(phi))
    err = tu.rel(a, b)
    print(f"commuting diagram {err:.2e}")
    assert err < 1e-13
    for name, o in (("h1", P_h1), ("nd", P_nd), ("grad", G_f), ("grad_c", G_c)):
        s = tu.copy_spread(o, ru.vector(o.nc, 3))
        print(f"copies of a shared dof, {name}: {s:.2e}")
        assert s < 1e-13
        assert o.inv_mult.min() < 1.0  # (there are shared dofs)


@pytest.mark.parametrize("kind", ru.MESHES)
def test_rotated_meshes_give_negative_signs_and_partial_waves(kind):
    for p in range(1, 6):
        neg = (tu.space(kind, "nd", p).elem_sign_lex < 0).mean()
        assert 0.1 < neg < 0.9, (p, neg)
    ne = ru.mesh(kind).ne
    for pf in range(1, 6):
        epw = tu.elems_per_wave(pf)
        assert epw == (16, 7, 4, 2, 1)[pf - 1]
        if kind == "ogrid15":  # a partial wave where a wave holds several elements, a partial block at every order
            assert ne % (4 * epw) != 0 and (epw == 1 or ne % epw != 0)
    if kind == "cyl80":  # whole blocks at orders 3 and 4
        assert ne % (4 * tu.elems_per_wave(3)) == 0 and ne % (4 * tu.elems_per_wave(4)) == 0
