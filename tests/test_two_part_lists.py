"""Keeps the lists of the two-part kernels (PA_MIXED2_CASE, PA_ERROR2_CASE in palace_amd/csrc/pa_mixed_hex2.hip, PA_RT2_CASE in
pa_rt_hex2.hip) inside PA_HEX_PQ_LIST and the new entry points in the public header.  CPU only."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "palace_amd", "csrc")
LISTS = (("PA_MIXED2_CASE", "pa_mixed_hex2.hip"), ("PA_ERROR2_CASE", "pa_mixed_hex2.hip"), ("PA_RT2_CASE", "pa_rt_hex2.hip"))
NEW_SYMBOLS = ("pa_op_two_rhs", "pa_error_op_apply_add2", "pa_error_op_two_parts")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _pairs(macro, source):
    return [(int(p), int(q)) for p, q in re.findall(macro + r"\(\s*(\d+)\s*,\s*(\d+)\s*\)", _read(CSRC, source))]


def _hex_pq():
    body = re.search(r"#define PA_HEX_PQ_LIST\(X, \.\.\.\)(.*?)\n#define", _read(CSRC, "pa_hex_core.hpp"), re.S).group(1)
    return [(int(p), int(q)) for p, q in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,", body)]


@pytest.mark.parametrize("macro,source", LISTS)
def test_two_part_lists(macro, source):
    pairs, pq = _pairs(macro, source), _hex_pq()
    assert len(pq) == 10
    assert pairs and len(set(pairs)) == len(pairs)
    assert set(pairs) <= set(pq), sorted(set(pairs) - set(pq))
    assert {(1, 2), (2, 3), (3, 4)} <= set(pairs)


def test_resource_table_covers_the_lists():
    """profiles/r11_two_part_resources.txt has a line for every compiled instantiation, none with scratch or spills."""
    lines = [l for l in _read(ROOT, "profiles", "r11_two_part_resources.txt").splitlines() if "_kernel<" in l and not l.startswith("#")]
    for l in lines:
        assert " scratch=0 " in l and " sspill=0 " in l and " vspill=0 " in l, l
    for kernels, (macro, source), per_pair in ((("mixed_hex_apply2_kernel", "mixed_hex_apply_pair_kernel"), LISTS[0], 2),
                                               (("mixed_hex_error2_kernel",), LISTS[1], 2), (("rt_hex_apply2_kernel",), LISTS[2], 3)):
        for p, q in _pairs(macro, source):
            assert sum(f"{k}<{p}, {q}," in l for l in lines for k in kernels) == per_pair, (kernels, p, q)
    assert len(lines) == 2 * len(_pairs(*LISTS[0])) + 2 * len(_pairs(*LISTS[1])) + 3 * len(_pairs(*LISTS[2]))


def test_new_symbols_are_declared_and_defined():
    header = re.sub(r"/\*.*?\*/", "", _read(ROOT, "include", "palace_amd.h"), flags=re.S)
    capi = _read(CSRC, "pa_capi.hip")
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert re.search(r"^int " + name + r"\s*\(", capi, re.M), name
