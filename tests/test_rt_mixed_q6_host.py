"""The six-point Raviart-Thomas and two-space kernels (palace_amd/csrc/pa_rt_hex_q6.hip, pa_mixed_hex_q6.hip) on the CPU: the
support predicate reads PA_HEX_Q6_LIST and the pair lists are what they were, the case lists of tests/test_rt_mixed_q6_gpu.py
cover every pair, the lane-to-line map and the LDS layout of both kernels at (5, 6) restated with numpy (HexLayout of
pa_hex_core.hpp with the passes of pa_rt_hex_core.hpp / pa_mixed_hex_core.hpp), and the committed resource table."""
import os
import re

import numpy as np

from tests import rthex_util as ru
from tests.test_hex_q6_host import _list, _read


def test_predicate_lists_and_routes():
    core = _read("pa_hex_core.hpp")
    q6, pq = _list("PA_HEX_Q6_LIST"), _list("PA_HEX_PQ_LIST")
    assert q6 == [(p, 6) for p in range(1, 6)]
    assert pq == [(1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4), (1, 5), (2, 5), (3, 5), (4, 5)]
    # the two lists, textually
    assert ("#define PA_HEX_PQ_LIST(X, ...)                                                                                       \\\n"
            "  X(1, 2, __VA_ARGS__) X(1, 3, __VA_ARGS__) X(2, 3, __VA_ARGS__) X(1, 4, __VA_ARGS__) X(2, 4, __VA_ARGS__)           \\\n"
            "  X(3, 4, __VA_ARGS__) X(1, 5, __VA_ARGS__) X(2, 5, __VA_ARGS__) X(3, 5, __VA_ARGS__) X(4, 5, __VA_ARGS__)\n") in core
    assert ("#define PA_HEX_Q6_LIST(X, ...) \\\n"
            "  X(1, 6, __VA_ARGS__) X(2, 6, __VA_ARGS__) X(3, 6, __VA_ARGS__) X(4, 6, __VA_ARGS__) X(5, 6, __VA_ARGS__)\n\n") in core
    body = re.search(r"inline bool hex_q6_supported\(int p, int q1d\) \{(.*?)\n\}", core, re.S).group(1)
    assert "PA_HEX_Q6_LIST(PA_HEX_PQ_LABEL, ) return true;" in body
    # both kernels and both dispatchers read the list; the five-point files route six points to them
    for f in ("pa_rt_hex_q6.hip", "pa_mixed_hex_q6.hip"):
        assert "PA_HEX_Q6_LIST(PA_HEX_PQ_CALL" in _read(f)
    assert "if (so.q1d == 6) return launch_rt_hex_q6(" in _read("pa_rt_hex.hip")
    assert "if (so.q1d == 6) return launch_mixed_hex_q6(" in _read("pa_mixed_hex.hip")
    # the three guards accept either list, with the messages they had
    capi, rt = _read("pa_capi.hip"), _read("pa_rt_hex.hip")
    assert 'if (!hex_pq_supported(b.order, b.q1d) && !hex_q6_supported(b.order, b.q1d)) throw hex_pq_error("H(div)"' in capi
    assert ('if (!hex_pq_supported(b1.order, b1.q1d) && !hex_q6_supported(b1.order, b1.q1d)) throw hex_pq_error("H(curl) - H(div)"'
            in capi)
    assert ('PA_REQUIRE(hex_pq_supported(so.p, so.q1d) || hex_q6_supported(so.p, so.q1d), "no H(div) hex kernel for this order '
            'and quadrature rule");') in rt
    # both files are built
    srcs = re.search(r"^SRCS = (.*)$", _read("Makefile"), re.M).group(1).split()
    assert "pa_rt_hex_q6.hip" in srcs and "pa_mixed_hex_q6.hip" in srcs


def test_gpu_cases_cover_every_pair():
    from tests import test_rt_mixed_q6_gpu as tq

    q6 = _list("PA_HEX_Q6_LIST")
    assert tq.Q6 == q6 and tq.Q1D == 6
    assert {p for k, p in tq.CASES if k == "ogrid15"} == {p for p, _ in q6}
    assert ("cyl80", 5) in tq.CASES and len(set(tq.CASES)) == len(tq.CASES)
    # at six points the 15-element mesh leaves the fourth workgroup with three live waves, the 80-element one whole workgroups
    assert ru.mesh("ogrid15").ne == 15 and ru.mesh("cyl80").ne == 80 and 15 % 4 == 3 and 80 % 4 == 0


# ---- the layouts at (5, 6), restated ---------------------------------------------------------------
P1, Q1 = 5, 6
NC, T = P1 + 1, Q1 * Q1
A_FIELD, B_FIELD = Q1 * NC * NC, Q1 * Q1 * NC


class Layout:
    """HexLayout<5, 6, BASE, NA, NB> of pa_hex_core.hpp."""

    def __init__(self, base, na, nb):
        self.base, self.na, self.nb = base, na, nb
        self.elem = base + na * A_FIELD + nb * B_FIELD
        self.elem_pad = ((self.elem + 15) // 16 * 16) | 16

    def ia(self, f, qx, j, k):
        return self.base + f * A_FIELD + (qx * NC + j) * NC + k

    def ib(self, f, qx, qy, k):
        return self.base + self.na * A_FIELD + f * B_FIELD + (qx * Q1 + qy) * NC + k


def _stores(L, nfields, sizes, base):
    """{pass: [(lane, slot)]} of the stores of one component with (NX, NY, NZ) = sizes whose dofs start at `base` (forward X, Y;
    transposed Z, Y; the result slots), `nfields` chains per buffer."""
    nx, ny, nz = sizes
    out = {"X": [], "Y": [], "Zt": [], "Yt": [], "out": []}
    for lane in range(T):
        ta, tb = lane % Q1, lane // Q1
        for q in range(Q1):
            if ta < ny and tb < nz:  # lane (j, k)
                out["X"] += [(lane, L.ia(f, q, ta, tb)) for f in range(nfields)]
            if tb < nz:  # lane (qx, k)
                out["Y"] += [(lane, L.ib(f, ta, q, tb)) for f in range(nfields)]
        for k in range(nz):  # lane (qx, qy)
            out["Zt"] += [(lane, L.ib(f, ta, tb, k)) for f in range(nfields)]
        for j in range(ny):
            if tb < nz:
                out["Yt"] += [(lane, L.ia(f, ta, j, tb)) for f in range(nfields)]
        if ta < ny and tb < nz:
            out["out"] += [(lane, base + i + nx * (ta + ny * tb)) for i in range(nx)]
    return out


def _check_component_passes(L, nfields, comps, ndofs):
    for C, (sizes, base) in enumerate(comps):
        assert max(sizes) <= Q1  # a line per lane in every pass
        for name, st in _stores(L, nfields, sizes, base).items():
            slots = np.array([s for _, s in st])
            assert len(set(slots.tolist())) == len(slots), (C, name)  # no slot twice within a pass
            lo = 0 if name == "out" else L.base
            assert slots.min() >= lo and slots.max() < L.elem, (C, name)  # inside the element's buffers, below the tables
    res = np.concatenate([[s for _, s in _stores(L, nfields, sizes, base)["out"]] for sizes, base in comps])
    assert np.array_equal(np.sort(res), np.arange(ndofs))  # the three components' result slots tile [0, P) once
    npl = -(-ndofs // T)
    m = np.array([t + T * r for t in range(T) for r in range(npl) if t + T * r < ndofs])
    assert np.array_equal(np.sort(m), np.arange(ndofs))  # every dof is gathered and stored by exactly one (lane, round)
    # the A buffers (after X) and the B buffers (after Y) do not overlap
    assert L.ia(L.na - 1, Q1 - 1, NC - 1, NC - 1) < L.ib(0, 0, 0, 0) and L.ib(L.nb - 1, Q1 - 1, Q1 - 1, NC - 1) == L.elem - 1


def _comps(closed_along_c):
    """((NX, NY, NZ), offset) of the three components: closed (p + 1 nodes) along c and open along the others, or the reverse."""
    nl, nt = (NC, P1) if closed_along_c else (P1, NC)
    return [(tuple(nl if d == C else nt for d in range(3)), C * nl * nt * nt) for C in range(3)]


def _launch_bytes(src, waves_name, strip, layout):
    waves = int(re.search(r"constexpr int " + waves_name + r" = (\d+);", src).group(1))
    assert waves == 4
    assert f"static constexpr int ELEM = {layout}<P1, Q1>::ELEM_PAD;" in src
    assert "static constexpr int STRIDE = ELEM + ((TAB + 1) & ~1);" in src
    assert "smem + (size_t)wave * S::STRIDE" in src
    assert f"sizeof(double) * (size_t){waves_name} * {strip}<P1, Q1>::STRIDE" in src
    assert f"__launch_bounds__(64 * {waves_name}, 1)" in src
    assert "if (e >= a.ne) return" in src and "if (lane >= L::T) return" in src and 64 // T == 1
    assert "__syncthreads" not in src and not re.search(r"atomic\w*\(", src, re.I)  # wave-level syncs, plain stores
    return waves


def test_rt_lane_map_and_lds_layout_at_order_five():
    src, core = _read("pa_rt_hex_q6.hip"), _read("pa_rt_hex_core.hpp")
    assert "using RTLayout = HexLayout<P1, Q1, 3 * P1 * P1 * (P1 + 1), 2, 2>;" in core
    P = 3 * P1 * P1 * NC
    L = Layout(P, 2, 2)
    assert "static constexpr int TAB = Q1 * (P1 + 2 * (P1 + 1));" in src
    tab = Q1 * (P1 + 2 * NC)
    stride = L.elem_pad + ((tab + 1) & ~1)
    assert (P, L.elem, L.elem_pad, tab, stride) == (450, 1314, 1328, 102, 1430)
    _check_component_passes(L, 2, _comps(True), P)
    waves = _launch_bytes(src, "kRTQ6Waves", "RTQ6Strip", "RTLayout")
    assert 8 * waves * stride == 45760 < 64 * 1024
    # the table view points behind the element's pad: [Bo | Bc | Gc]
    assert "tab.Bo = sm + S::ELEM, tab.Bc = tab.Bo + Q1 * P1, tab.Gc = tab.Bc + Q1 * (P1 + 1);" in src
    assert L.elem <= L.elem_pad and L.elem_pad + tab <= stride


def test_mixed_lane_map_and_lds_layout_at_order_five():
    src, core = _read("pa_mixed_hex_q6.hip"), _read("pa_mixed_hex_core.hpp")
    assert "using MHLayout = HexLayout<P1, Q1, 3 * P1 * (P1 + 1) * (P1 + 1), 1, 1>;" in core
    P_nd, P_rt = 3 * P1 * NC * NC, 3 * P1 * P1 * NC
    L = Layout(P_nd, 1, 1)
    assert "static constexpr int TAB = Q1 * (P1 + (P1 + 1));" in src
    tab = Q1 * (P1 + NC)
    stride = L.elem_pad + ((tab + 1) & ~1)
    assert (P_nd, P_rt, L.elem, L.elem_pad, tab, stride) == (540, 450, 972, 976, 66, 1042)
    _check_component_passes(L, 1, _comps(False), P_nd)  # the Nedelec side: open along c
    _check_component_passes(L, 1, _comps(True), P_rt)   # the Raviart-Thomas side shares the buffers, its dofs fill [0, 450)
    waves = _launch_bytes(src, "kMHQ6Waves", "MHQ6Strip", "MHLayout")
    assert 8 * waves * stride == 33344 < 64 * 1024
    assert "tab.Bo = sm + S::ELEM, tab.Bc = tab.Bo + Q1 * P1;" in src
    # the element sum of the error form: lane t stores slot t, lane 0 adds the 36 in order and is the one writer
    assert T <= L.base and "sm[t] = err;" in src and "for (int i = 0; i < T; i++) sum += sm[i];" in src
    assert "a.out[a.eorder ? a.eorder[e] : e] += sum;" in src and "__shfl" not in src


def test_resource_table_has_every_instantiation_without_sgpr_spills():
    with open(os.path.join(ru.ROOT, "profiles", "r15_rt_mixed_q6_resources.txt")) as f:
        lines = [ln for ln in f.read().splitlines() if "_q6_" in ln and "vgpr=" in ln]
    b = ("true", "false")
    want = [f"rt_hex_q6_kernel<{p}, 6, {v}, {d}, {qd}>" for p in range(1, 6) for v, d in (("true", "false"), ("false", "true"),
            ("true", "true")) for qd in b]
    want += [f"mixed_hex_q6_{k}_kernel<{p}, 6, {nd}>" for p in range(1, 6) for k in ("apply", "error") for nd in b]
    assert len(want) == 50 and len(lines) == 50
    for name in want:
        hit = [ln for ln in lines if name in ln]
        assert len(hit) == 1, name
        assert re.search(r"\bsspill=0\b", hit[0]), hit[0]
    # so neither object carries the flag that keeps SGPR spills out of VGPR lanes
    for ln in _read("Makefile").splitlines():
        if "amdgpu-spill-sgpr-to-vgpr" in ln and not ln.startswith("#"):
            assert "_q6" not in ln
    # the packed forms of the RT kernel and the four two-space kernels have no scratch
    for ln in lines:
        packed_rt = re.search(r"rt_hex_q6_kernel<\d, 6, (true|false), (true|false), true>", ln)
        if packed_rt or "mixed_hex_q6_" in ln:
            assert re.search(r"\bscratch=0\b", ln), ln
