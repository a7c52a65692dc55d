"""The case table of the dense MFMA element kernels (palace_amd/csrc/pa_dense.hip): one case per compiled instantiation that an input
can reach, with the cell it must land in.  tests/test_dense_instantiations.py keeps the table in step with the source (CPU),
tests/test_dense_cells_gpu.py runs every case against the oracle and asserts the cell through `Operator.dense_kernel()`.

A cell is (form, PT, mode, geometry form):
  form      "resident" (tables in LDS), "staged", "split" (resident, split-vector input), "complex" (resident, two parts per pass)
  PT        16 PT = the padded dof count of an element
  mode      the DenseMode name
  geometry  "curved" | "affine" | "list" (a mesh with affine and curved blocks: one launch of the affine-list kernel and one of the
            curved-list kernel); "-" for the staged kernel, which reads the geometry factors of every point whatever they are

Most cases are synthetic: the kernel takes any element's tables (the header of pa_dense.hip), so a case is random [qcomp Q x P]
tables, random offsets and a random restriction of the wanted kind over real (straight or curved quadratic) simplices, sized to
land in its cell by the host's own arithmetic, which `lds_bytes` / `resident_fits` / `affine_fits` restate.  The natural elements
that reach a newly covered cell cheaply are listed in NATURAL."""
from dataclasses import dataclass, field

import numpy as np

KEB = 16  # elements per block
PTS = (1, 2, 3, 4, 6, 9)  # kPT of pa_dense_host.hpp
RES_PTS = (1, 2, 3, 4, 6)  # the PT switch of the resident launcher
SMALL_PTS = (1, 2, 3)  # affine, list, split and complex kernels
MODES = ("CURL", "VMASS", "CURLMASS", "DIFF", "DIFFMASS", "MASS", "CURL2", "VMASS2", "CURLMASS2", "DIFF2", "DIFFMASS2", "VMASS1",
         "DIFF1", "DIFFMASS1")
MODES_3D, MODES_2D, MODES_1D = MODES[:6], MODES[6:11], MODES[11:]
SPLIT_MODES = ("CURL", "VMASS", "CURLMASS", "DIFF")
GEOS = ("curved", "affine", "list")
# mode -> (vector element?, element dimension, value components, derivative components)
MODE_INFO = {"CURL": (True, 3, 0, 3), "VMASS": (True, 3, 3, 0), "CURLMASS": (True, 3, 3, 3), "DIFF": (False, 3, 0, 3),
             "DIFFMASS": (False, 3, 1, 3), "MASS": (False, 3, 1, 0), "CURL2": (True, 2, 0, 1), "VMASS2": (True, 2, 2, 0),
             "CURLMASS2": (True, 2, 2, 1), "DIFF2": (False, 2, 0, 2), "DIFFMASS2": (False, 2, 1, 2), "VMASS1": (True, 1, 1, 0),
             "DIFF1": (False, 1, 0, 1), "DIFFMASS1": (False, 1, 1, 1)}
WAVES = {"staged": 4, "curved": 8, "affine": 12}  # waves per workgroup


# ---- the host's arithmetic (pa_dense_host.hpp; tests/test_dense_host.py compares the two value by value) ----------------------
def pt_of(P):
    for v in PTS:
        if P <= 16 * v:
            return v
    raise ValueError("more than 144 dofs")


def stride(PT):
    return 16 * PT + (2 if PT & 1 else 18)


def lds_bytes(PT, nct, Q, curl):
    rows = (Q + 15) // 16 * nct * 16
    return 8 * (rows * stride(PT) + (8 * 4 * PT * 64 if curl else 0))


def resident_fits(PT, nct, Q, curl):
    return PT in RES_PTS and lds_bytes(PT, nct, Q, curl) <= 150 * 1024


def affine_fits(PT, nct, Q, curl):
    rows, Q4 = (Q + 15) // 16 * nct * 16, (Q + 3) // 4 * 4
    return PT <= 3 and Q > 1 and 8 * ((Q4 + 31) // 32 * 32 + rows * stride(PT) + (12 * 4 * PT * 64 if curl else 0)) <= 160 * 1024


@dataclass(frozen=True)
class Case:
    id: str
    form: str
    PT: int
    mode: str
    geo: str
    P: int = 0
    Q: int = 0
    ne: int = 40
    dim: int = 0  # element dimension (MASS serves 3, 2 and 1)
    sdim: int = 0
    restr: str = "plain"  # "plain" | "signs" | "curl" (tridiagonal, entries -1 / 0 / 1)
    staged_by: str = ""  # "env" (PALACE_AMD_DENSE=staged) | "lds" (tables overflow) | "nonsym" (non-symmetric coefficient) |
    #                      "pt9" (more than 96 dofs: no resident kernel, whatever the tables' size)
    rows: bool = False  # so few elements in so large a space that an accumulating apply goes through the block's row list
    hdiv: str = ""  # "" | "mass" | "divdiv" | "divdivmass": an H(div) block that runs on this mode's arithmetic
    imag: str = ""  # complex form: the mode of the imaginary operator
    natural: str = ""  # the kind of natural element natural_inputs builds ("" = synthetic) and its arguments
    extra: dict = field(default_factory=dict, hash=False, compare=False)

    @property
    def cell(self):
        return (self.form, self.PT, self.mode, "-" if self.form == "staged" else self.geo)

    @property
    def nct(self):
        return MODE_INFO[self.mode][2] + MODE_INFO[self.mode][3]

    @property
    def n_straight(self):
        """Leading elements with a constant Jacobian: none, all, or whole blocks making up at least a quarter of the blocks."""
        if self.geo in ("curved", "-"):
            return 0
        if self.geo == "affine":
            return self.ne
        nb = (self.ne + KEB - 1) // KEB
        return KEB * ((nb + 3) // 4)

    @property
    def lists(self):
        nb = (self.ne + KEB - 1) // KEB
        return (self.n_straight // KEB, nb - self.n_straight // KEB) if self.geo == "list" else (0, 0)

    def setup_cells(self):
        """The set-up and diagonal kernels this case runs besides its apply kernel."""
        contra3 = self.hdiv == "divdivmass"
        out = set()
        if self.form != "staged":
            if self.dim == 1:
                out.add(("qdata1", self.mode, self.sdim))
            elif self.dim == 3 and self.mode == "CURL2":
                out.add(("qdata2", "CURL2", 11))
            elif self.dim == 2:
                out.add(("qdata2", self.mode, 8 if self.sdim == 3 else 6))
            else:
                out.add(("qdata", self.mode))
        if self.form in ("resident", "staged"):  # (the split and complex cases compare applies only)
            out.add(("diag", self.mode) if self.dim == 3 and self.mode in MODES_3D and not contra3 else ("diag_qd", self.mode))
        return out


def _pick(PT, mode, geo, curl_wanted, exact):
    """(P, Q, restriction) of a synthetic resident case: the padded size less three dofs (padding slots) and a point count that is no
    multiple of 4, or (`exact`) 16 PT dofs and a multiple of 16 points; two chunks of points where the tables still fit, and
    the restriction asked for unless its exchange buffer takes the LDS the tables need."""
    vec, _, nci, ncd = MODE_INFO[mode]
    nct = nci + ncd
    P = 16 * PT if exact else 16 * PT - 3
    kinds = (["curl", "signs"] if curl_wanted else ["signs"]) if vec else ["plain"]
    for restr in kinds:
        for Q in ((32, 16) if exact else (27, 13)):
            ok = resident_fits(PT, nct, Q, restr == "curl") and (geo == "curved" or affine_fits(PT, nct, Q, restr == "curl"))
            if ok:
                return P, Q, restr
    raise ValueError((PT, mode, geo))


_MASS_DIMS = ((3, 3), (2, 2), (2, 3), (1, 2), (1, 3))


def _dims(mode, k):
    dim = MODE_INFO[mode][1]
    if mode == "MASS":
        return _MASS_DIMS[k % 5]
    return (dim, 3) if dim == 3 else (dim, 2 + k % 2)


def _overflow_q(PT, nct):
    nch = 1
    while lds_bytes(PT, nct, 16 * nch, False) <= 150 * 1024:
        nch += 1
    return 16 * nch - 3


def _build():
    cases = []
    # ---- resident: every PT x mode x geometry form
    for mi, mode in enumerate(MODES):
        k = 0
        for geo in GEOS:
            for PT in (RES_PTS if geo == "curved" else SMALL_PTS):
                dim, sdim = _dims(mode, k)
                P, Q, restr = _pick(PT, mode, geo, (PT + mi) % 2 == 0, False)
                ne = 40 if geo != "list" else 69
                cases.append(Case(f"res-{mode}-pt{PT}-{geo}", "resident", PT, mode, geo, P, Q, ne, dim, sdim, restr))
                k += 1
    # ---- staged: PT <= 3 through the switch (the resident case above is its twin), larger elements through tables that overflow
    # the LDS; a non-symmetric material at PT = 4 and 6; PT = 9 also with tables that WOULD fit (no resident kernel of that size)
    for mi, mode in enumerate(MODES_3D):
        vec, _, nci, ncd = MODE_INFO[mode]
        for PT in PTS:
            restr = ("curl" if (PT + mi) % 2 else "signs") if vec else "plain"
            if PT <= 3:
                cases.append(Case(f"staged-{mode}-pt{PT}-env", "staged", PT, mode, "-", 16 * PT - 3, 27, 40, 3, 3, restr, "env"))
            else:
                Q = _overflow_q(PT, nci + ncd)
                cases.append(Case(f"staged-{mode}-pt{PT}-lds", "staged", PT, mode, "-", 16 * PT - 3, Q, 24, 3, 3, restr, "lds"))
    for PT in (4, 6):
        cases.append(Case(f"staged-VMASS-pt{PT}-nonsym", "staged", PT, "VMASS", "-", 16 * PT - 3, 13, 40, 3, 3, "signs", "nonsym"))
        cases.append(Case(f"staged-DIFFMASS-pt{PT}-nonsym", "staged", PT, "DIFFMASS", "-", 16 * PT, 16, 40, 3, 3, "plain", "nonsym"))
    cases.append(Case("staged-MASS-pt9-small", "staged", 9, "MASS", "-", 141, 13, 24, 3, 3, "plain", "pt9"))
    cases.append(Case("staged-VMASS-pt9-small", "staged", 9, "VMASS", "-", 144, 16, 24, 3, 3, "signs", "pt9"))
    # ---- once per form: exactly 16 PT dofs (no padding slot) and a multiple of 16 points
    for PT, mode, geo in ((2, "CURLMASS", "curved"), (4, "CURLMASS2", "curved"), (6, "DIFFMASS", "curved"), (3, "CURL", "affine"),
                          (2, "DIFFMASS2", "affine"), (1, "VMASS", "list"), (3, "DIFF2", "list")):
        dim, sdim = _dims(mode, PT)
        P, Q, restr = _pick(PT, mode, geo, True, True)
        cases.append(Case(f"res-{mode}-pt{PT}-{geo}-exact", "resident", PT, mode, geo, P, Q, 69 if geo == "list" else 40, dim, sdim, restr))
    cases.append(Case("staged-CURLMASS-pt2-env-exact", "staged", 2, "CURLMASS", "-", 32, 32, 40, 3, 3, "curl", "env"))
    cases.append(Case("staged-DIFF-pt6-lds-exact", "staged", 6, "DIFF", "-", 96, 16 * ((_overflow_q(6, 3) + 15) // 16), 24, 3, 3, "plain", "lds"))
    # ---- element-count edges, one mode per form: one element, one whole block, a block and one element, and one element more
    # than a workgroup's waves have blocks (surplus waves, a partial last block, fewer blocks than waves)
    for form, geo, PT, mode, restr in (("staged", "-", 3, "CURLMASS", "curl"), ("resident", "curved", 2, "CURL", "curl"),
                                       ("resident", "affine", 3, "VMASS", "signs"), ("resident", "curved", 4, "VMASS2", "signs"),
                                       ("resident", "curved", 6, "DIFF", "plain")):
        nw = WAVES["staged" if form == "staged" else geo]
        for ne in (1, 16, 17, 16 * nw + 1):
            dim, sdim = (2, 3) if mode == "VMASS2" else (3, 3)
            cases.append(Case(f"edge-{form}-{mode}-pt{PT}-{geo}-ne{ne}", form, PT, mode, geo, 16 * PT - 3, 13, ne, dim, sdim, restr,
                              "env" if form == "staged" else ""))
    # a mesh with affine and curved blocks whose last (curved) block is partial and whose lists are shorter than a workgroup
    cases.append(Case("edge-resident-DIFFMASS-pt1-list-ne33", "resident", 1, "DIFFMASS", "list", 13, 13, 33, 3, 3, "plain"))
    # ---- a block that touches few dofs of a large space adds through its row list
    cases.append(Case("rows-resident-VMASS2-pt3-curved", "resident", 3, "VMASS2", "curved", 45, 13, 20, 2, 3, "signs", rows=True))
    cases.append(Case("rows-staged-CURL-pt4-lds", "staged", 4, "CURL", "-", 61, _overflow_q(4, 3), 20, 3, 3, "curl", "lds", rows=True))
    # ---- H(div) blocks on the arithmetic of an existing mode (the tables change places, the D takes the contravariant map)
    cases.append(Case("rt-mass-pt2-list", "resident", 2, "CURL", "list", 29, 13, 69, 3, 3, "signs", hdiv="mass"))
    cases.append(Case("rt-mass-pt4-curved", "resident", 4, "CURL", "curved", 61, 13, 40, 3, 3, "signs", hdiv="mass"))
    cases.append(Case("rt-divdiv-pt3-curved", "resident", 3, "CURL2", "curved", 45, 13, 40, 3, 3, "signs", hdiv="divdiv"))
    cases.append(Case("rt-divdiv-pt1-affine", "resident", 1, "CURL2", "affine", 13, 13, 40, 3, 3, "signs", hdiv="divdiv"))
    cases.append(Case("rt-divdivmass-pt2-curved", "resident", 2, "DIFFMASS", "curved", 29, 13, 40, 3, 3, "signs", hdiv="divdivmass"))
    cases.append(Case("rt-divdivmass-pt6-curved", "resident", 6, "DIFFMASS", "curved", 93, 13, 40, 3, 3, "signs", hdiv="divdivmass"))
    cases.append(Case("rt-tri-mass-pt1-affine", "resident", 1, "VMASS2", "affine", 13, 13, 40, 2, 2, "signs", hdiv="mass"))
    # ---- split-vector input: PT <= 3, four modes, every block curved or every block affine
    for mi, mode in enumerate(SPLIT_MODES):
        for PT in SMALL_PTS:
            for geo in ("curved", "affine"):
                P, Q, restr = _pick(PT, mode, geo, (PT + mi) % 2 == 0, False)
                cases.append(Case(f"split-{mode}-pt{PT}-{geo}", "split", PT, mode, geo, P, Q, 40, 3, 3, restr))
    # ---- complex form: curl-curl + mass with an imaginary mass, curl-curl or curl-curl + mass operator on the same blocks
    for PT in SMALL_PTS:
        for gi, geo in enumerate(GEOS):
            P, Q, restr = _pick(PT, "CURLMASS", geo, (PT + gi) % 2 == 0, False)
            cases.append(Case(f"complex-pt{PT}-{geo}", "complex", PT, "CURLMASS", geo, P, Q, 69 if geo == "list" else 40, 3, 3, restr,
                              imag=("VMASS", "CURL", "CURLMASS")[(PT + gi) % 3]))
    return cases


SYNTHETIC = _build()

# Natural elements (palace_amd.fem spaces on small meshes, natural_inputs below)
NATURAL = [
    # the reference's default rule on order-4 Nedelec tetrahedra: 84 dofs, 125 points
    Case("nd-tet-p4-default-rule-CURL", "staged", 6, "CURL", "-", 84, 125, 48, 3, 3, "curl", "lds", natural="nd_tet", extra=dict(p=4, rule="default", kind="tet10")),
    Case("nd-tet-p4-default-rule-CURLMASS", "staged", 6, "CURLMASS", "-", 84, 125, 48, 3, 3, "curl", "lds", natural="nd_tet", extra=dict(p=4, rule="default", kind="tet10")),
    # the same element with the 14-point rule: the one natural way into the resident kernel at PT = 6
    Case("nd-tet-p4-14-points-VMASS", "resident", 6, "VMASS", "curved", 84, 14, 48, 3, 3, "curl", natural="nd_tet", extra=dict(p=4, rule=5, kind="tet10")),
    Case("nd-tet-p4-14-points-CURL", "resident", 6, "CURL", "curved", 84, 14, 48, 3, 3, "curl", natural="nd_tet", extra=dict(p=4, rule=5, kind="tet4")),
    # H1 tetrahedra with straight sides: the affine form of the three H1 modes
    Case("h1-tet-p2-affine-DIFF", "resident", 1, "DIFF", "affine", 10, 27, 48, 3, 3, "plain", natural="h1_tet", extra=dict(p=2, kind="tet4")),
    Case("h1-tet-p3-affine-DIFFMASS", "resident", 2, "DIFFMASS", "affine", 20, 64, 48, 3, 3, "plain", natural="h1_tet", extra=dict(p=3, kind="tet4")),
    Case("h1-tet-p4-affine-MASS", "resident", 3, "MASS", "affine", 35, 125, 48, 3, 3, "plain", natural="h1_tet", extra=dict(p=4, kind="tet4")),
    Case("h1-tet-p5-curved-DIFF", "resident", 4, "DIFF", "curved", 56, 24, 48, 3, 3, "plain", natural="h1_tet", extra=dict(p=5, kind="tet10", rule=6)),
    # Raviart-Thomas tetrahedra of order 4 (70 dofs): mass on the curl-curl arithmetic, div-div, div-div + mass
    Case("rt-tet-p4-14-points-mass", "resident", 6, "CURL", "curved", 70, 14, 48, 3, 3, "signs", hdiv="mass", natural="rt_tet", extra=dict(p=4, rule=5, kind="tet10")),
    Case("rt-tet-p4-default-rule-mass", "staged", 6, "CURL", "-", 70, 125, 48, 3, 3, "signs", "lds", hdiv="mass", natural="rt_tet", extra=dict(p=4, rule="default", kind="tet10")),
    Case("rt-tet-p4-default-rule-divdiv", "resident", 6, "CURL2", "curved", 70, 125, 48, 3, 3, "signs", hdiv="divdiv", natural="rt_tet", extra=dict(p=4, rule="default", kind="tet10")),
    Case("rt-tet-p4-14-points-divdivmass", "resident", 6, "DIFFMASS", "curved", 70, 14, 48, 3, 3, "signs", hdiv="divdivmass", natural="rt_tet", extra=dict(p=4, rule=5, kind="tet4")),
    Case("rt-tet-p2-divdivmass-affine", "resident", 1, "DIFFMASS", "affine", 15, 14, 48, 3, 3, "signs", hdiv="divdivmass", natural="rt_tet", extra=dict(p=2, rule=5, kind="tet4")),
    # triangles of orders 4 and 5 on the first 208 elements of the reference's cavity2d mesh: straight (vertex geometry) and warped
    Case("nd-tri-p4-CURLMASS2", "resident", 2, "CURLMASS2", "affine", 24, 25, 208, 2, 2, "signs", natural="tri", extra=dict(p=4, space="nd")),
    Case("nd-tri-p5-VMASS2", "resident", 3, "VMASS2", "curved", 35, 36, 208, 2, 2, "signs", natural="tri", extra=dict(p=5, space="nd")),
    Case("nd-tri-p5-CURL2", "resident", 3, "CURL2", "affine", 35, 36, 208, 2, 2, "signs", natural="tri", extra=dict(p=5, space="nd")),
    Case("h1-tri-p4-DIFF2", "resident", 1, "DIFF2", "curved", 15, 25, 208, 2, 2, "plain", natural="tri", extra=dict(p=4, space="h1")),
    Case("h1-tri-p5-DIFFMASS2", "resident", 2, "DIFFMASS2", "affine", 21, 36, 208, 2, 2, "plain", natural="tri", extra=dict(p=5, space="h1")),
]

CASES = SYNTHETIC + NATURAL
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"


# ---- every compiled cell -------------------------------------------------------------------------------------------------------
def compiled_apply_cells(res_modes=MODES, res_pts=RES_PTS, split_modes=SPLIT_MODES, split_pts=SMALL_PTS, cplx_pts=SMALL_PTS,
                         staged_modes=MODES_3D, staged_pts=PTS):
    """What the launchers of pa_dense.hip instantiate, from the lists the CPU test parses out of the source.  PA_RES_CASE names
    <PT, MODE, false>, <PT, MODE, PT <= 3>, <PT, MODE, false, false, PT <= 3> and <PT, MODE, PT <= 3, false, PT <= 3>: four kernels
    for PT <= 3 (curved, affine, curved-list + affine-list = "list"), one and the same for PT = 4 and 6."""
    cells = set()
    for mode in res_modes:
        for PT in res_pts:
            cells.add(("resident", PT, mode, "curved"))
            if PT <= 3:
                cells |= {("resident", PT, mode, "affine"), ("resident", PT, mode, "list")}
    for mode in split_modes:
        for PT in split_pts:
            cells |= {("split", PT, mode, "curved"), ("split", PT, mode, "affine")}
    for PT in cplx_pts:
        cells |= {("complex", PT, "CURLMASS", g) for g in GEOS}
    for mode in staged_modes:
        for PT in staged_pts:
            cells.add(("staged", PT, mode, "-"))
    return cells


# A cell may stand here only when a rule of make_dense_sub or of a launcher shuts it out for EVERY input; the entry names the rule.
# Every compiled apply cell is reachable, so the map is empty; what the rules shut out are combinations that are not compiled:
NOT_COMPILED = {
    "affine / list / split / complex at PT > 3": "affine_fits: the affine flags need PT <= 3; dense_kernel_cell and launch_resident_mode: "
                                                 "SMALL = PT <= 3; dense_split_ok and dense_complex_ok: PT <= 3",
    "2-D and line modes in the staged form": "make_dense_sub: PA_REQUIRE((dim == 3 && mode < MODE_CURL2 && !contra) || d_L); PA_DENSE_CASE lists the "
                                             "six 3-D modes",
    "resident form at PT = 9": "make_dense_sub keeps blocks of more than 96 dofs on the staged kernel: launch_dense_apply has no resident case 9",
    "split form of the H1 pair, the H1 mass, the 2-D and the line modes": "resident_split_mode: CURL, VMASS, CURLMASS, DIFF",
    "complex form of any mode but CURLMASS": "dense_complex_ok: dr.mode == MODE_CURLMASS",
}
EXCLUDED = {}

# Cells that a test compared with a reference before this table existed (worked out from the sizes, rules and restrictions those
# tests use, through the arithmetic above; a cell they may have reached without saying which geometry form ran is not claimed)
TESTS_BEFORE = {
    "tet": "tests/test_tet_gpu.py::test_nd_tet_apply",
    "tetl": "tests/test_tet_gpu.py::test_nd_tet_apply_partly_curved_mesh",
    "h1tet": "tests/test_tet_gpu.py::test_h1_tet_apply",
    "hex": "tests/test_dense_gpu.py::test_dense_apply_and_diagonal",
    "bdr": "tests/test_tet_gpu.py::test_nd_tet_boundary_mass, ::test_nd_tet_boundary_curlcurl_and_pair",
    "hexb": "tests/test_dense_gpu.py::test_hex_boundary_mass[3]",
    "surf": "tests/test_2d_gpu.py::test_h1_apply_2d_and_surface",
    "line": "tests/test_line_gpu.py::test_line_element_forms",
    "split": "tests/test_split_gpu.py::test_split_apply_dense_tetrahedra",
    "cplx": "tests/test_complex_gpu.py::test_fused_complex_apply_tets",
}


def _before():
    B = {}
    for PT in SMALL_PTS:
        for mode in ("CURL", "VMASS", "CURLMASS"):
            B[("resident", PT, mode, "list")] = "tetl"
            if not (mode == "CURLMASS" and PT == 3):  # (its 64-point rule and exchange buffer overflow the LDS: staged there)
                B[("resident", PT, mode, "affine")] = B[("resident", PT, mode, "curved")] = "tet"
            B[("split", PT, mode, "affine")] = "split"
        for mode in ("DIFF", "MASS", "DIFFMASS"):
            if not (mode == "DIFFMASS" and PT == 3):
                B[("resident", PT, mode, "curved")] = "h1tet"
        for geo in GEOS:
            if not (PT == 1 and geo == "list"):
                B[("complex", PT, "CURLMASS", geo)] = "cplx"
    B[("split", 1, "DIFF", "affine")] = B[("split", 2, "DIFF", "affine")] = "split"
    for mode in ("CURL", "VMASS", "CURLMASS", "DIFF", "MASS"):
        B[("resident", 4, mode, "curved")] = "hex"
    for mode in ("CURL2", "VMASS2", "CURLMASS2"):
        B[("resident", 1, mode, "affine")] = B[("resident", 1, mode, "curved")] = "bdr"
    B[("resident", 2, "VMASS2", "curved")] = "hexb"
    B[("resident", 1, "DIFF2", "curved")] = B[("resident", 1, "DIFFMASS2", "curved")] = "surf"
    for mode in MODES_1D:
        B[("resident", 1, mode, "curved")] = "line"
    B[("staged", 3, "CURLMASS", "-")], B[("staged", 3, "DIFFMASS", "-")] = "tet", "h1tet"
    for mode in ("CURL", "VMASS", "CURLMASS", "DIFF", "DIFFMASS"):
        B[("staged", 4, mode, "-")] = "hex"
    for mode in ("CURL", "VMASS", "CURLMASS"):
        B[("staged", 9, mode, "-")] = "hex"
    return B


BEFORE = _before()


def design_table():
    """The coverage table of DESIGN.md section 3.5 (the CPU test holds the document to it): for every compiled apply cell the key of
    the earlier test that covered it, `new` where tests/test_dense_cells_gpu.py is the first, or `excl` with its rule in EXCLUDED."""
    have = {c.cell for c in CASES}

    def mark(cell):
        if cell in EXCLUDED:
            return "excl"
        assert cell in have, cell
        return BEFORE.get(cell, "new")

    cols = [("curved", PT) for PT in RES_PTS] + [("affine", PT) for PT in SMALL_PTS] + [("list", PT) for PT in SMALL_PTS]
    lines = ["| resident | " + " | ".join(f"{g} {PT}" for g, PT in cols) + " |", "|---" * (len(cols) + 1) + "|"]
    for mode in MODES:
        lines.append(f"| {mode} | " + " | ".join(mark(("resident", PT, mode, g)) for g, PT in cols) + " |")
    lines += ["", "| staged | " + " | ".join(f"PT {PT}" for PT in PTS) + " |", "|---" * (len(PTS) + 1) + "|"]
    for mode in MODES_3D:
        lines.append(f"| {mode} | " + " | ".join(mark(("staged", PT, mode, "-")) for PT in PTS) + " |")
    cols = [(g, PT) for g in ("curved", "affine") for PT in SMALL_PTS]
    lines += ["", "| split | " + " | ".join(f"{g} {PT}" for g, PT in cols) + " |", "|---" * (len(cols) + 1) + "|"]
    for mode in SPLIT_MODES:
        lines.append(f"| {mode} | " + " | ".join(mark(("split", PT, mode, g)) for g, PT in cols) + " |")
    cols = [(g, PT) for g in GEOS for PT in SMALL_PTS]
    lines += ["", "| complex | " + " | ".join(f"{g} {PT}" for g, PT in cols) + " |", "|---" * (len(cols) + 1) + "|"]
    lines.append("| CURLMASS | " + " | ".join(mark(("complex", PT, "CURLMASS", g)) for g, PT in cols) + " |")
    return lines


# ---- inputs (numpy only: the CPU test builds them too, to check each case's cell against the host's arithmetic) ------------------
class Inputs:
    """Everything a case hands to the library and to the oracle: nodes / elem_nodes / attr / grad [dim, Q, npe] / w (geometry),
    J [ne, Q, sdim, dim], interp / deriv (None where the mode has no such table), offsets, orients, curl_orients, lsize, touched."""


def p2_grad_table(dim, x):
    """Gradients of the quadratic Lagrange basis of the reference simplex at points x [Q, dim]: [dim, Q, npe], nodes = the
    vertices, then the midpoints of the vertex pairs (a, b), a < b, in lexicographic order."""
    l = np.concatenate([1 - x.sum(axis=1, keepdims=True), x], axis=1)  # [Q, dim + 1]
    dl = np.concatenate([-np.ones((1, dim)), np.eye(dim)])  # [dim + 1, dim]
    pairs = [(a, b) for a in range(dim + 1) for b in range(a + 1, dim + 1)]
    G = np.zeros((dim, x.shape[0], dim + 1 + len(pairs)))
    for i in range(dim + 1):
        G[:, :, i] = (4 * l[:, i] - 1)[None, :] * dl[i][:, None]
    for k, (a, b) in enumerate(pairs):
        G[:, :, dim + 1 + k] = 4 * (l[:, a][None, :] * dl[b][:, None] + l[:, b][None, :] * dl[a][:, None])
    return G, pairs


def simplices(rng, ne, dim, sdim, n_straight):
    """ne quadratic simplices of dimension dim in sdim-space, each with nodes of its own: random well-shaped straight ones with
    their mid-side nodes at the exact midpoints; from element n_straight on the mid-side nodes are displaced (curved elements)."""
    h = 0.4
    pairs = [(a, b) for a in range(dim + 1) for b in range(a + 1, dim + 1)]
    A = h * (np.eye(sdim)[:, :dim][None] + 0.25 * rng.uniform(-1, 1, (ne, sdim, dim)))
    V = np.empty((ne, dim + 1, sdim))
    V[:, 0] = rng.uniform(-0.3, 0.3, (ne, sdim))  # (near the origin: the Jacobian of a straight element cancels to fewer roundings)
    for d in range(dim):
        V[:, d + 1] = V[:, 0] + A[:, :, d]
    mids = np.stack([0.5 * (V[:, a] + V[:, b]) for a, b in pairs], axis=1)
    bend = 0.03 * h * rng.uniform(-1, 1, mids.shape)
    bend[:n_straight] = 0.0
    X = np.concatenate([V, mids + bend], axis=1)  # [ne, npe, sdim]
    npe = X.shape[1]
    return X.reshape(ne * npe, sdim), np.arange(ne * npe, dtype=np.int32).reshape(ne, npe)


def curl_orientations(rng, ne, P):
    """Tridiagonal element transformations with entries in {-1, 0, 1}, in 2 x 2 blocks on a random half of the dof pairs (the
    values MFEM's ND_DofTransformation produces; as in tests/test_dense_gpu.py)."""
    cor = np.zeros((ne, P, 3), dtype=np.int8)
    cor[:, :, 1] = rng.choice([-1, 1], size=(ne, P))
    pairs = rng.random((ne, P // 2)) < 0.5
    for k in range(P // 2):
        sel = pairs[:, k]
        v = rng.integers(-1, 2, size=(ne, 4)).astype(np.int8)
        a, b = 2 * k, 2 * k + 1
        cor[sel, a, 1], cor[sel, a, 2] = v[sel, 0], v[sel, 1]
        cor[sel, b, 0], cor[sel, b, 1] = v[sel, 2], v[sel, 3]
    return cor


def table_shapes(case):
    """(components of the value table, of the derivative table) the library reads for this case (0: none)."""
    vec, dim, nci, ncd = MODE_INFO[case.mode]
    if case.hdiv == "mass":
        return case.dim, 0
    if case.hdiv in ("divdiv", "divdivmass"):
        return case.dim, 1
    return nci, ncd


def synthetic_inputs(case):
    import zlib

    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    I = Inputs()
    dim, sdim, ne, P, Q = case.dim, case.sdim, case.ne, case.P, case.Q
    I.nodes, I.elem_nodes = simplices(rng, ne, dim, sdim, case.n_straight)
    I.attr = (1 + np.arange(ne) % 2).astype(np.int32)
    bary = rng.dirichlet(np.ones(dim + 1), size=Q)  # interior points; the weights are any positive numbers
    I.x = np.ascontiguousarray(bary[:, 1:])
    I.w = rng.uniform(0.5, 1.5, Q) / (Q * (1, 2, 6)[dim - 1])
    I.grad, _ = p2_grad_table(dim, I.x)
    I.J = np.einsum("dqn,eni->eqid", I.grad, I.nodes[I.elem_nodes])
    nci, ncd = table_shapes(case)
    I.interp = rng.uniform(-1, 1, (nci, Q, P)) if nci else None
    I.deriv = rng.uniform(-1, 1, (ncd, Q, P)) if ncd else None
    # offsets: P distinct dofs per element out of the first `reach` of the space; the last five dofs belong to no element
    reach = max(P + 7, ne * P // 3) if not case.rows else 4 * ne * P + 50
    I.offsets = np.stack([rng.choice(reach, size=P, replace=False) for _ in range(ne)]).astype(np.int32)
    I.lsize = reach + 5
    I.orients = (rng.random((ne, P)) < 0.5) if case.restr == "signs" else None
    I.curl_orients = curl_orientations(rng, ne, P) if case.restr == "curl" else None
    return I


def geometry_form(J):
    """curved | affine | list as make_dense_sub will find it: a block of 16 elements is affine when all its elements have a constant
    Jacobian; the lists are used when at least a quarter of the blocks, and not all, are affine.  The device compares the packed D
    to 1e-13; elements whose Jacobian varies between 1e-14 and 1e-9 are refused here (neither clearly straight nor curved)."""
    ne = J.shape[0]
    v = np.abs(J - J[:, :1]).reshape(ne, -1).max(axis=1) / np.abs(J).reshape(ne, -1).max(axis=1)
    assert not np.any((v > 1e-14) & (v < 1e-9)), "elements that are neither clearly straight nor clearly curved"
    nb = (ne + KEB - 1) // KEB
    flags = [bool(np.all(v[KEB * b:KEB * (b + 1)] <= 1e-14)) for b in range(nb)]
    na = sum(flags)
    return "affine" if na == nb else ("list" if na * 4 >= nb else "curved"), (na, nb - na)


def _warp(X):
    x, y = X[:, 0], X[:, 1]
    z = X[:, 2] if X.shape[1] == 3 else 0.3 * x
    out = [x + 0.04 * np.sin(2 * y + z), y + 0.05 * x * z + 0.03 * x * x, z - 0.03 * np.cos(3 * x) * y]
    return np.stack(out[:X.shape[1]], axis=1)


def natural_inputs(case):
    """Spaces of palace_amd.fem on small meshes: the 48 tetrahedra of a 2 x 2 x 2 cube (straight tet4 or warped tet10), the first 208
    triangles of the cavity2d golden mesh (vertex geometry, or its tri6 nodes warped)."""
    import os

    from palace_amd.fem import tet, tri

    I = Inputs()
    ex = case.extra
    if case.natural in ("nd_tet", "h1_tet", "rt_tet"):
        mesh = tet.cube_tet_mesh(2)
        mesh.attr[:] = 1 + np.arange(mesh.ne) % 2
        if ex["kind"] == "tet10":
            m2 = tet.to_quadratic(mesh, _warp)
            m2.attr[:] = mesh.attr
            mesh = m2
        p, rule = ex["p"], ex.get("rule")
        I.x, I.w = tet.default_tet_rule(p) if rule == "default" else (tet.tet_quadrature_symmetric(rule) if rule else tet.tet_quadrature(p + 1))
        if case.natural == "rt_tet":
            from palace_amd.fem import rt

            sp = rt.RTTetSpace(mesh, p)
        else:
            sp = tet.NDTetSpace(mesh, p) if case.natural == "nd_tet" else tet.H1TetSpace(mesh, p)
        I.interp, I.deriv = sp.elem.tables(I.x)
        I.offsets, I.lsize = sp.offsets, sp.ndofs
        I.orients = I.curl_orients = None
        if case.natural == "rt_tet":
            I.orients = sp.orients
        if case.natural == "nd_tet":
            if sp.diagonal_transform:
                I.orients = sp.orients
            else:
                I.curl_orients = sp.curl_orients
        I.nodes, I.elem_nodes, I.attr = mesh.nodes, mesh.elem_nodes, mesh.attr
        I.grad = mesh.geometry_grad_table(I.x)
    else:
        M_ = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cavity2d_mesh.npz"))
        en = M_["elem_nodes"].astype(np.int64)
        used, inv = np.unique(en[:, :3], return_inverse=True)
        full = tri.TriMesh(M_["nodes"][used], inv.reshape(-1, 3), 1 + np.arange(en.shape[0]) % 2, elem_nodes=en, nodes=M_["nodes"])
        p, ne = ex["p"], case.ne
        sp = tri.NDTriSpace(full, p) if ex["space"] == "nd" else tri.H1TriSpace(full, p)
        I.x, I.w = tri.tri_quadrature(p + 1)
        I.interp, I.deriv = sp.elem.tables(I.x)
        dofs, off = np.unique(sp.offsets[:ne], return_inverse=True)  # the dofs of the first ne elements, renumbered
        I.offsets, I.lsize = off.reshape(ne, -1).astype(np.int32), int(dofs.size)
        I.orients = sp.orients[:ne] if ex["space"] == "nd" else None
        I.curl_orients = None
        I.attr = full.attr[:ne]
        if case.geo == "affine":  # vertex geometry: constant Jacobians to the bit
            lin = tri.TriMesh(full.verts, full.tris)
            I.nodes, I.elem_nodes, I.grad = lin.nodes, lin.elem_nodes[:ne], lin.geometry_grad_table(I.x)
        else:
            L = np.ptp(full.nodes[:, 0])
            I.nodes, I.elem_nodes, I.grad = L * _warp(full.nodes / L), full.elem_nodes[:ne], full.geometry_grad_table(I.x)
    I.nodes = np.ascontiguousarray(I.nodes, dtype=np.float64)
    I.elem_nodes = np.ascontiguousarray(I.elem_nodes, dtype=np.int32)
    I.deriv = np.asarray(I.deriv)
    if I.deriv.ndim == 2:
        I.deriv = I.deriv[None]
    I.J = np.einsum("dqn,eni->eqid", I.grad, I.nodes[I.elem_nodes])
    nci, ncd = table_shapes(case)
    if not nci:
        I.interp = None
    if not ncd:
        I.deriv = None
    return I


def qfunction(case):
    """(name of the library's QFunction constant in palace_amd.ceed, name of the oracle's in palace_oracle, eval modes as letters:
    I interp, G grad, C curl, D div, W weight, contexts as letters: 1 scalar, M matrix of the space dimension; two letters: a pair
    context in that order)."""
    s = case.sdim
    two = {2: "22", 3: "32"}.get(s)
    line = {2: "21", 3: "31"}.get(s)
    if case.hdiv == "mass":
        return ("QF_HDIV_33", "QF_HDIV", "I", "M") if case.dim == 3 else (f"QF_HDIV_{two}", f"QF_HDIV_{two}", "I", "M")
    if case.hdiv == "divdiv":
        return "QF_L2_1", "QF_L2_1", "DW", "1"
    if case.hdiv == "divdivmass":
        return "QF_L2MASS_33", "QF_L2MASS", "IDW", "M1"
    return {"CURL": ("QF_HDIV_33", "QF_HDIV", "C", "M"), "VMASS": ("QF_HCURL_33", "QF_HCURL", "I", "M"),
            "CURLMASS": ("QF_HDIVMASS_33", "QF_HDIVMASS", "CI", "MM"), "DIFF": ("QF_HCURL_33", "QF_HCURL", "G", "M"),
            "DIFFMASS": ("QF_HCURLMASS_33", "QF_HCURLMASS", "GI", "1M"), "MASS": ("QF_H1_1", "QF_H1MASS", "I", "1"),
            "CURL2": ("QF_L2_1", "QF_L2_1", "CW", "1"), "VMASS2": (f"QF_HCURL_{two}", f"QF_HCURL_{two}", "I", "M"),
            "CURLMASS2": (f"QF_HDIVMASS_{two}", f"QF_HDIVMASS_{two}", "CIW", "M1"), "DIFF2": (f"QF_HCURL_{two}", f"QF_HCURL_{two}", "G", "M"),
            "DIFFMASS2": (f"QF_HCURLMASS_{two}", f"QF_HCURLMASS_{two}", "GI", "1M"),
            "VMASS1": (f"QF_HCURL_{line}", "QF_HCURL_LINE", "I", "M"), "DIFF1": (f"QF_HCURL_{line}", "QF_HCURL_LINE", "G", "M"),
            "DIFFMASS1": (f"QF_HCURLMASS_{line}", "QF_HCURLMASS_LINE", "GI", "1M")}[case.mode]


def inputs(case):
    I = natural_inputs(case) if case.natural else synthetic_inputs(case)
    I.touched = np.zeros(I.lsize, dtype=bool)
    I.touched[np.asarray(I.offsets).ravel()] = True
    return I


def predicted_cell(case, I):
    """The cell make_dense_sub and the launchers will choose for these inputs (the arithmetic restated above)."""
    ne, P = np.asarray(I.offsets).shape
    Q = len(I.w)
    PT = pt_of(P)
    curl = I.curl_orients is not None
    resident = case.staged_by not in ("env", "nonsym") and resident_fits(PT, case.nct, Q, curl)
    if not resident:
        return ("staged", PT, case.mode, "-"), (0, 0)
    geo, lists = geometry_form(I.J)
    if geo != "curved" and not affine_fits(PT, case.nct, Q, curl):
        geo = "curved"
    form = case.form if case.form in ("split", "complex") else "resident"
    return (form, PT, case.mode, geo), (lists if geo == "list" else (0, 0))
