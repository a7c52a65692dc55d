"""The six-point pair list (PA_HEX_Q6_LIST, palace_amd/csrc/pa_hex_core.hpp) against the case lists of
tests/test_hex_q6_gpu.py, and the lane-to-line map and LDS layout of the H(curl) kernel at (5, 6) (pa_nd_hex_q6.hip with
NDLayout of pa_nd_hex_core.hpp) restated with numpy: within a pass no two working lanes store to one slot, nothing is stored
outside the element's buffers, and the wave's strip is what the launch allocates.  CPU only."""
import os
import re

import numpy as np

from tests import rthex_util as ru

CSRC = os.path.join(ru.ROOT, "palace_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _list(name):
    body = re.search(r"#define " + name + r"\(X, \.\.\.\)(.*?)\n\n", _read("pa_hex_core.hpp"), re.S).group(1)
    return [(int(p), int(q)) for p, q in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,", body)]


def test_pair_list_and_parity_cases():
    from tests import test_hex_q6_gpu as tq

    q6, pq = _list("PA_HEX_Q6_LIST"), _list("PA_HEX_PQ_LIST")
    assert sorted(q6) == [(p, 6) for p in range(1, 6)] and len(set(q6)) == len(q6)
    assert len(pq) == 10 == len(set(pq)) and not set(q6) & set(pq)
    for lst in (tq.ND_PQ, tq.H1_PQ):
        assert set(q6) <= set(lst) and len(set(lst)) == len(lst)
    # every pair meets every variant of the H(curl) matrix, and order 5 the whole-block mesh
    assert {(p, v) for k, p, v in tq.ND_CASES if k == "ogrid15"} == {(p, v) for p, _ in q6 for v in tq.VARIANTS}
    assert ("cyl80", 5, "default") in tq.ND_CASES and len(tq.VARIANTS) == 7
    # both kernels and both dispatchers read the list
    for f in ("pa_nd_hex_q6.hip", "pa_h1_hex_q6.hip"):
        assert "PA_HEX_Q6_LIST(PA_HEX_PQ_CALL" in _read(f)
    assert "so.q1d == 6" in _read("pa_nd_hex.hip") and "so.q1d == 6" in _read("pa_h1_hex.hip")


# ---- the layout at (5, 6), restated ----------------------------------------------------------------
P1, Q1 = 5, 6
NC, T = P1 + 1, Q1 * Q1
SJ, SQ, TY, TQ = NC, NC * NC, NC, NC * Q1  # NDStrides<5, 6>: the dense strides
A_FIELD, B_FIELD = SQ * Q1, TQ * Q1
ELEM = 2 * A_FIELD + 3 * B_FIELD
ELEM_PAD = ((ELEM + 15) // 16 * 16) | 16
TAB = Q1 * (P1 + 2 * NC)
STRIDE = ELEM_PAD + ((TAB + 1) & ~1)


def ia(f, qx, j, k):
    return f * A_FIELD + qx * SQ + j * SJ + k


def ib(f, qx, qy, k):
    return 2 * A_FIELD + f * B_FIELD + qx * TQ + qy * TY + k


def _sizes(C):
    return (P1 if C == 0 else NC), (P1 if C == 1 else NC), (P1 if C == 2 else NC)


def _stores(C):
    """{pass: [(lane, slot)]} of the stores of component C (forward X, Y; transposed Z, Y; the result slots)."""
    ni, nj, nk = _sizes(C)
    out = {"X": [], "Y": [], "Zt": [], "Yt": [], "out": []}
    for lane in range(T):
        ta, tb = lane % Q1, lane // Q1
        for q in range(Q1):
            if ta < nj and tb < nk:  # lane (j, k)
                out["X"] += [(lane, ia(f, q, ta, tb)) for f in range(2)]
            if tb < nk:  # lane (qx, k)
                out["Y"] += [(lane, ib(f, ta, q, tb)) for f in range(3)]
        for k in range(nk):  # lane (qx, qy)
            out["Zt"] += [(lane, ib(f, ta, tb, k)) for f in range(3)]
        for j in range(nj):
            if tb < nk:
                out["Yt"] += [(lane, ia(f, ta, j, tb)) for f in range(2)]
        if ta < nj and tb < nk:
            out["out"] += [(lane, C * P1 * NC * NC + i + ni * (ta + nj * tb)) for i in range(ni)]
    return out


def test_lane_map_and_lds_layout_at_order_five():
    src = _read("pa_nd_hex_q6.hip")
    assert (ELEM, ELEM_PAD, TAB, STRIDE) == (1080, 1104, 102, 1206)
    # 36 working lanes of 64, one element per wave
    assert 64 // T == 1 and re.search(r"if \(lane >= L::T\) return;", src)
    for C in range(3):
        for name, st in _stores(C).items():
            slots = np.array([s for _, s in st])
            assert len(set(slots.tolist())) == len(slots), (C, name)  # no slot twice within a pass
            assert slots.min() >= 0 and slots.max() < ELEM, (C, name)  # inside the element's buffers, below the tables
    # the three components' result slots tile [0, P) exactly once: what the sorted-order store reads through perm
    res = np.concatenate([[s for _, s in _stores(C)["out"]] for C in range(3)])
    assert np.array_equal(np.sort(res), np.arange(3 * P1 * NC * NC))
    # every dof is gathered and stored by exactly one (lane, round)
    PP = 3 * P1 * NC * NC
    npl = -(-PP // T)
    m = np.array([t + T * r for t in range(T) for r in range(npl) if t + T * r < PP])
    assert np.array_equal(np.sort(m), np.arange(PP)) and npl == 15
    # the A buffers (after X) and the B buffers (after Y) do not overlap; the table copy starts past the element's pad
    assert ia(1, Q1 - 1, NC - 1, NC - 1) < ib(0, 0, 0, 0) and ib(2, Q1 - 1, Q1 - 1, NC - 1) == ELEM - 1 < ELEM_PAD
    # the strip of a wave as the kernel and the launch spell it
    waves = int(re.search(r"constexpr int kQ6Waves = (\d+);", src).group(1))
    assert waves == 4
    assert "static constexpr int ELEM = NDLayout<P1, Q1>::ELEM_PAD;" in src
    assert "static constexpr int TAB = Q1 * (P1 + 2 * (P1 + 1));" in src
    assert "static constexpr int STRIDE = ELEM + ((TAB + 1) & ~1);" in src
    assert "smem + (size_t)wave * S::STRIDE" in src
    assert "sizeof(double) * (size_t)kQ6Waves * NDQ6Strip<P1, Q1>::STRIDE" in src
    assert 8 * waves * STRIDE == 38592 < 64 * 1024  # bytes per workgroup: below the limit that needs the attribute ...
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src  # ... which the launch sets above it
    # NDLayout<5, 6> is the generic (dense-stride) layout: no specialisation of the strides for this pair
    core = _read("pa_nd_hex_core.hpp")
    assert not re.search(r"struct NDStrides<\s*5\s*,\s*6\s*>", core) and not re.search(r"struct NDLayout<\s*5\s*,\s*6\s*>", core)
