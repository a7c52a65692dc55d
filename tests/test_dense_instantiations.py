"""Keeps the case table of the dense MFMA element kernels (tests/dense_cases.py, run on the GPU by tests/test_dense_cells_gpu.py) in
step with the instantiations palace_amd/csrc/pa_dense.hip compiles: every (form, PT, mode, geometry form) a launcher can start, and
every set-up and diagonal kernel, must have a case or stand in EXCLUDED with the rule that shuts it out.  And the inputs of every
case are built here and pushed through the host's arithmetic as dense_cases.py states it (tests/test_dense_host.py holds that
statement to palace_amd/csrc/pa_dense_host.hpp, value by value), so that a case whose stated cell is not the one make_dense_sub
will choose fails without a GPU.  CPU only."""
import os
import re

import pytest

from tests import dense_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name="pa_dense.hip"):
    with open(os.path.join(ROOT, "palace_amd", "csrc", name)) as f:
        return f.read()


def _modes(src, macro):
    """The MODE_ arguments of the uses of one X-macro (its #define has the bare parameter MODE and does not match)."""
    return [m for m in re.findall(r"\b%s\(MODE_(\w+)\)" % macro, src)]


def _parse():
    src, host = _src(), _src("pa_dense_host.hpp")  # (the modes and the element sizes live in the host header)
    P = {}
    enum = re.search(r"enum DenseMode \{(.*?)\};", host, re.S).group(1)
    P["enum"] = [(n, int(v)) for n, v in re.findall(r"MODE_(\w+) = (\d+)", enum)]
    P["kPT"] = [int(v) for v in re.search(r"constexpr int kPT\[\] = \{([^}]*)\}", host).group(1).split(",")]
    for macro in ("PA_RES_CASE", "PA_RES_SPLIT_CASE", "PA_DENSE_CASE", "PA_QD1_CASE", "PA_QD2_CASE", "PA_QD_CASE", "PA_DIAG_CASE",
                  "PA_DIAG2_CASE"):
        P[macro] = _modes(src, macro)
    P["res_pt"] = [int(v) for v in re.findall(r"case (\d+): launch_resident_pt<\1>\(ds, a, s\)", src)]
    P["split_pt"] = sorted({int(v) for v in re.findall(r"launch_resident_split<(\d+)>\(ds, a, s\)", src)})
    P["cplx_pt"] = [int(v) for v in re.findall(r"case (\d+): launch_resident_mode<\1, MODE_CURLMASS, true, false>\(dr, a, s\)", src)]
    # the one launch helper: every resident instantiation is one of the four geometry forms launch_resident_mode names
    P["cell_forms"] = re.findall(r"launch_resident_cell<PT, MODE, (\w+), CPLX, (\w+), SPLIT>", src)
    P["staged_pt"] = [int(v) for v in re.findall(r"case (\d+): launch_pt<\1>\(ds, a, s\)", src)]
    P["qd1_sdim"] = sorted({int(v) for v in re.findall(r"dense_qdata1_kernel<MODE, (\d+)>", src)})
    P["qd2_rows"] = sorted({int(v) for v in re.findall(r"dense_qdata2_kernel<MODE, (\d+)>", src)})
    P["qd2_3d"] = re.findall(r"dense_qdata2_kernel<MODE_(\w+), (\d+)>", src)
    P["src"] = src
    return P


def _compiled(P):
    apply_cells = dc.compiled_apply_cells(P["PA_RES_CASE"], P["res_pt"], P["PA_RES_SPLIT_CASE"], P["split_pt"], P["cplx_pt"],
                                          P["PA_DENSE_CASE"], P["staged_pt"])
    setup = {("qdata", m) for m in P["PA_QD_CASE"]}
    setup |= {("qdata1", m, s) for m in P["PA_QD1_CASE"] for s in P["qd1_sdim"]}
    setup |= {("qdata2", m, n) for m in P["PA_QD2_CASE"] for n in P["qd2_rows"]}
    setup |= {("qdata2", m, int(n)) for m, n in P["qd2_3d"]}
    setup |= {("diag", m) for m in P["PA_DIAG_CASE"]} | {("diag_qd", m) for m in P["PA_DIAG2_CASE"]}
    return apply_cells, setup


def uncovered(cases, P=None):
    """The compiled cells, apply kernels first, that neither a case nor EXCLUDED accounts for."""
    apply_cells, setup = _compiled(P or _parse())
    have = {c.cell for c in cases}
    have_setup = set().union(*[c.setup_cells() for c in cases]) if cases else set()
    return sorted(apply_cells - have - set(dc.EXCLUDED), key=str) + sorted(setup - have_setup - set(dc.EXCLUDED), key=str)


def test_the_source_lists_are_found_and_are_the_expected_ones():
    """A regular expression that finds nothing, or a list that grew, fails here before the coverage test can pass for nothing."""
    P = _parse()
    assert [n for n, _ in P["enum"]] == list(dc.MODES) and [v for _, v in P["enum"]] == list(range(14))
    assert tuple(P["kPT"]) == dc.PTS
    counts = {k: len(P[k]) for k in ("PA_RES_CASE", "PA_RES_SPLIT_CASE", "PA_DENSE_CASE", "PA_QD1_CASE", "PA_QD2_CASE", "PA_QD_CASE",
                                     "PA_DIAG_CASE", "PA_DIAG2_CASE")}
    assert counts == {"PA_RES_CASE": 14, "PA_RES_SPLIT_CASE": 4, "PA_DENSE_CASE": 6, "PA_QD1_CASE": 4, "PA_QD2_CASE": 6, "PA_QD_CASE": 6,
                      "PA_DIAG_CASE": 6, "PA_DIAG2_CASE": 10}, counts
    for k in counts:
        assert len(set(P[k])) == len(P[k]), k
    assert tuple(P["PA_RES_CASE"]) == dc.MODES and tuple(P["PA_DENSE_CASE"]) == dc.MODES_3D
    assert tuple(P["PA_RES_SPLIT_CASE"]) == dc.SPLIT_MODES
    assert tuple(P["res_pt"]) == dc.RES_PTS and tuple(P["staged_pt"]) == dc.PTS
    assert tuple(P["split_pt"]) == dc.SMALL_PTS == tuple(P["cplx_pt"])
    assert P["qd1_sdim"] == [2, 3] and P["qd2_rows"] == [6, 8] and P["qd2_3d"] == [("CURL2", "11")]
    apply_cells, setup = _compiled(P)
    # resident 5 x 14 curved + 3 x 14 x {affine, list}, split 3 x 4 x 2, complex 3 x 3, staged 6 x 6
    assert len(apply_cells) == 70 + 84 + 24 + 9 + 36
    assert len(setup) == 6 + 8 + 12 + 1 + 6 + 10
    # the forms compiled_apply_cells counts per (PT, mode): affine-list and curved-list (PT <= 3), affine (PT <= 3), curved
    assert P["cell_forms"] == [("SMALL", "SMALL"), ("false", "SMALL"), ("SMALL", "false"), ("false", "false")]
    assert "constexpr bool SMALL = PT <= 3;" in P["src"] and "if constexpr (!SPLIT)" in P["src"]
    # (the host's arithmetic that dense_cases.py restates is compared value by value in tests/test_dense_host.py)
    src = P["src"]
    assert "constexpr int kDenseWaves = 4;" in src and "constexpr int kResWaves = 8;" in src and "constexpr int kAffWaves = 12;" in src
    assert dc.WAVES == {"staged": 4, "curved": 8, "affine": 12}


def test_every_compiled_cell_has_a_case_or_a_rule_that_excludes_it():
    P = _parse()
    apply_cells, setup = _compiled(P)
    missing = uncovered(dc.CASES, P)
    assert not missing, "compiled, but neither in tests/dense_cases.py nor in EXCLUDED: %s" % missing
    stray = sorted({c.cell for c in dc.CASES} - apply_cells, key=str)
    assert not stray, "cases that claim a cell no launcher starts: %s" % stray
    for cell, rule in dc.EXCLUDED.items():
        assert cell in apply_cells | setup and isinstance(rule, str) and len(rule) > 20, cell
        assert cell not in {c.cell for c in dc.CASES}, "excluded and run: %s" % (cell,)


def test_a_removed_case_is_reported_by_the_name_of_its_cell():
    P = _parse()
    for cell in (("resident", 6, "CURLMASS2", "curved"), ("staged", 9, "MASS", "-"), ("complex", 2, "CURLMASS", "list"),
                 ("split", 3, "DIFF", "curved")):
        assert uncovered([c for c in dc.CASES if c.cell != cell], P) == [cell]
    only = [c for c in dc.CASES if c.hdiv != "divdiv"]  # (the one way into dense_qdata2_kernel<MODE_CURL2, 11>)
    assert uncovered(only, P) == [("qdata2", "CURL2", 11)]


def test_design_md_table_agrees_with_the_case_table():
    """DESIGN.md section 3.5a gives, for every compiled cell, the earlier test, `new` or `excl`: the lines are those dense_cases.py
    makes from the case table, BEFORE and EXCLUDED."""
    apply_cells, _ = _compiled(_parse())
    assert set(dc.BEFORE) <= apply_cells and set(dc.BEFORE.values()) <= set(dc.TESTS_BEFORE)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        doc = f.read()
    for line in dc.design_table():
        assert line in doc, line
    new = sum(1 for c in apply_cells if c not in dc.BEFORE and c not in dc.EXCLUDED)
    assert f"{new} of the {len(apply_cells)} cells had no test" in doc
    assert ("**Excluded: nothing.**" in doc) == (not dc.EXCLUDED)
    for key in dc.TESTS_BEFORE:
        assert f"`{key}`" in doc, key


def test_the_case_table_follows_its_own_rules():
    ids = [c.id for c in dc.CASES]
    assert len(set(ids)) == len(ids)
    for c in dc.CASES:
        vec, dim, nci, ncd = dc.MODE_INFO[c.mode]
        assert c.form in ("resident", "staged", "split", "complex") and c.geo in dc.GEOS + ("-",), c.id
        assert (c.form == "staged") == (c.geo == "-") == bool(c.staged_by), c.id
        assert c.dim == dim or c.mode == "MASS" or (c.hdiv and c.dim == 3), c.id
        assert c.sdim == c.dim or (c.dim, c.sdim) in ((2, 3), (1, 2), (1, 3)), c.id
        assert c.ne <= 400 and c.P <= 144, c.id
    syn = dc.SYNTHETIC
    # per form: 16 PT - 3 dofs (padding slots) and exactly 16 PT; points once no multiple of 4 and once a multiple of 16
    for form, geo in (("resident", "curved"), ("resident", "affine"), ("resident", "list"), ("staged", "-")):
        sel = [c for c in syn if c.form == form and c.geo == geo]
        assert any(c.P == 16 * c.PT - 3 for c in sel) and any(c.P == 16 * c.PT and c.Q % 16 == 0 for c in sel), (form, geo)
        assert any(c.Q % 4 for c in sel), (form, geo)
    # element-count edges per form
    for form, geo, nw in (("staged", "-", 4), ("resident", "curved", 8), ("resident", "affine", 12)):
        nes = {c.ne for c in syn if c.form == form and c.geo == geo}
        assert {1, 16, 17, 16 * nw + 1} <= nes, (form, geo, sorted(nes))
    # the staged form under the switch for every PT <= 3 and each 3-D mode, next to a resident case of the same cell coordinates
    for mode in dc.MODES_3D:
        for PT in dc.SMALL_PTS:
            assert any(c.staged_by == "env" and c.PT == PT and c.mode == mode for c in syn), (mode, PT)
    # partly curved meshes: an H1 3-D mode, a plane mode, a boundary mode (sdim = 3) and an H(div) block
    lists = [c for c in syn if c.geo == "list" and c.form == "resident"]
    assert any(c.mode in ("DIFF", "DIFFMASS", "MASS") and c.dim == 3 for c in lists)
    assert any(c.dim == 2 and c.sdim == 2 for c in lists) and any(c.dim == 2 and c.sdim == 3 for c in lists)
    assert any(c.hdiv for c in lists)
    # both restrictions of vector elements at every PT of both forms
    for form, pts in (("resident", dc.RES_PTS), ("staged", dc.PTS)):
        for PT in pts:
            kinds = {c.restr for c in syn if c.form == form and c.PT == PT}
            assert {"plain", "signs", "curl"} <= kinds, (form, PT, kinds)


@pytest.mark.parametrize("chunk", range(8))
def test_every_case_lands_in_its_cell_by_the_hosts_arithmetic(chunk):
    """The inputs of each case (sizes, restriction kind, Jacobians) through pt_of / resident_fits / affine_fits / geometry_form."""
    bad = []
    for c in dc.CASES[chunk::8]:
        I = dc.inputs(c)
        cell, lists = dc.predicted_cell(c, I)
        if cell != c.cell or lists != c.lists:
            bad.append((c.id, c.cell, cell, c.lists, lists))
        ne, P = I.offsets.shape
        assert I.offsets.min() >= 0 and I.offsets.max() < I.lsize and (c.natural or not I.touched.all()), c.id
        assert c.rows == (ne * P * 4 < I.lsize), c.id
        assert (c.P, c.Q) == (P, len(I.w)), (c.id, P, len(I.w))
        assert I.elem_nodes.min() >= 0 and I.elem_nodes.max() < I.nodes.shape[0] and I.attr.min() >= 1, c.id
    assert not bad, bad
