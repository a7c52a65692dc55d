"""The kernels of palace_amd/csrc/csr_op.hip (k_csr_spmv, k_csr_spmv_step, k_csr_spmv_split, k_csr_eliminate, k_flag,
k_csr_diag) on matrices built to stress them: tests/cxx/csr_kernels_check.cpp -- a C++ program on the library's CsrOperator /
ParOperator with a long double reference and the derived bound (k_i + 8) 2^-53 S_i per row -- is built and run ONCE; the tests
below read its report, one group of cases each.  The program's header says what it builds and why."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASE = re.compile(r"^case (\S+):(\w+) rows (\d+) lanes (\d+) ratio (\S+) (OK|FAIL)$")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """Builds and runs the program; an abnormal end (a signal, a HIP error, an exception, a time limit) fails the fixture, so
    that nothing else of this module starts on the GPU."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("csr_kernels") / "csr_kernels_check")
    libdir = os.path.join(ROOT, "palace_amd", "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "palace_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "csr_kernels_check.cpp"),
                           "-L" + libdir, "-lpalace_amd", "-Wl,-rpath," + libdir, "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "PALACE_AMD_FUSED_STEP_CSR"}
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120, env=env)
    assert run.returncode in (0, 1), (run.returncode, run.stdout[-2000:], run.stderr[-2000:])  # 1: a comparison failed (below)
    cases, cover, summary = [], {}, None
    for ln in run.stdout.splitlines():
        m = _CASE.match(ln)
        if m:
            cases.append(dict(name=m.group(1), op=m.group(2), rows=int(m.group(3)), lanes=int(m.group(4)), ratio=float(m.group(5)),
                              ok=m.group(6) == "OK", line=ln))
        elif ln.startswith("coverage lanes "):
            w = ln.split()
            cover[int(w[2])] = {w[i]: int(w[i + 1]) for i in range(3, len(w), 2)}
        elif ln.startswith("summary "):
            summary = ln
    assert summary is not None and cases, run.stdout[-2000:]
    print(run.stdout)
    return dict(cases=cases, cover=cover, summary=summary, returncode=run.returncode)


def _group(report, ops, min_cases):
    sel = [c for c in report["cases"] if c["op"] in ops]
    assert len(sel) >= min_cases, (ops, len(sel))
    bad = [c["line"] for c in sel if not c["ok"] or not c["ratio"] <= 1.0]
    worst = max(c["ratio"] for c in sel)
    print(f"{'/'.join(ops)}: {len(sel)} cases, worst error / bound {worst:.3g}")
    assert not bad, bad
    for lanes in (4, 8, 16):
        assert any(c["lanes"] == lanes for c in sel), (ops, lanes)
    return sel


def test_every_instantiation_ran_on_the_shapes_that_stress_it(report):
    """CsrOperator::Lanes(): each matrix ran on the instantiation its nnz / nrows asks for (strict >: 12 n -> 4, 12 n + 1 -> 8,
    24 n -> 8, 24 n + 1 -> 16), and each of the three on an empty row, a row of 4 LPR + 1 entries and 256 / LPR -+ 1 rows."""
    sel = _group(report, ("lanes",), 40)
    th = {c["name"]: c["lanes"] for c in sel if c["name"].startswith("threshold/")}
    assert th == {"threshold/12n+0": 4, "threshold/12n+1": 8, "threshold/24n+0": 8, "threshold/24n+1": 16}, th
    for lanes in (4, 8, 16):
        assert report["cover"][lanes] == dict(empty_row=1, row_4lpr_plus_1=1, n_block_minus_1=1, n_block_plus_1=1), report["cover"]
        assert any(c["lanes"] == lanes and c["rows"] == 1 for c in sel)
    assert "coverage complete" in report["summary"]


def test_products(report):
    """Mult, MultValues, AddMult (a = 1, -0.7 into a non-zero y) on every matrix, rectangular ones included."""
    _group(report, ("mult", "multvalues", "addmult_1", "addmult_m0.7"), 160)


def test_transpose_diagonal_and_the_fused_form_switch(report):
    """MultTranspose = the bits of Mult on a matrix flagged symmetric and refused otherwise; AssembleDiagonal exact (0 without a
    stored diagonal entry, duplicates summed in storage order); PrepareChebyStep true for square matrices unless
    PALACE_AMD_FUSED_STEP_CSR=0."""
    _group(report, ("transpose",), 40)
    _group(report, ("diag",), 40)
    _group(report, ("prepare",), 40)


def test_eliminated_values(report):
    """EliminatedValues against the host selection, bit by bit: no / a third of / all rows essential, both diagonal values."""
    _group(report, ("eliminate",), 6)


def test_residual_and_smoother_step(report):
    """MultResidual(Values): res only, d0 only, both; MultChebyStep(Values): e_prev null / given, add, out in the buffer of
    e_prev; a result aliasing the multiplied vector is refused before any launch."""
    _group(report, ("residual",), 30)
    _group(report, ("step",), 30)
    _group(report, ("step_alias_refused",), 30)


def test_split_product(report):
    """MultSplit: n_true 0 / odd near n / 2 / n, the ghost buffer by the parity of the device counter (the other one poisoned),
    one buffer for both parities, with and without a second value array."""
    _group(report, ("split",), 30)


def test_par_operator_over_an_assembled_matrix(report):
    """ParOperator(CsrOperator), one rank, symmetric positive definite, both diagonal policies, against dense elimination: Mult
    through the eliminated values (x != y) and in place (the generic path), AddMult, AssembleDiagonal."""
    _group(report, ("par_mult", "par_mult_inplace", "par_addmult", "par_diag"), 24)


def test_repeated_runs_give_the_same_bits_and_no_guard_zone_is_written(report):
    _group(report, ("repro",), 40)
    assert "guards intact" in report["summary"], report["summary"]
    assert report["returncode"] == 0 and " failed 0 " in report["summary"], report["summary"]
