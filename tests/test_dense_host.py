"""Host half of the dense MFMA element kernels (palace_amd/csrc/pa_dense_host.hpp), checked on CPU: the index words, the packed
curl-orientation words, the transpose map of either E-vector layout and the table fragments against a plain C++ model of what the
kernels decode (tests/cpu/dense_host_check.cpp); and the plan -- PT, row stride, the two fit tests, the launch's LDS bytes, the
list rule -- swept over every size and compared with the arithmetic tests/dense_cases.py places its cases by."""
import os
import subprocess

import numpy as np
import pytest

from tests import dense_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "dense_host_check.cpp")
INC = os.path.join(ROOT, "palace_amd", "csrc")


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """The program's output: it exits non-zero when one of its own checks (the encodings) fails."""
    exe = str(tmp_path_factory.mktemp("dense_host") / "dense_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + INC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    return [l.split() for l in out.stdout.splitlines()]


def test_encodings_against_cpu_model(sweep):
    assert sweep and not [l for l in sweep if l[0] == "FAIL"]


def test_plan_agrees_with_the_case_tables_arithmetic(sweep):
    pts = [(int(l[1]), int(l[2])) for l in sweep if l[0] == "pt"]
    assert [P for P, _ in pts] == list(range(1, 146))
    for P, PT in pts:
        assert PT == (dc.pt_of(P) if P <= 144 else 0), (P, PT)
    plans = [[int(v) for v in l[1:]] for l in sweep if l[0] == "plan"]
    assert len(plans) == len(dc.PTS) * 6 * 400 * 2
    assert {(p[0], p[1], p[2], p[3]) for p in plans} == {(PT, nct, Q, c) for PT in dc.PTS for nct in range(1, 7) for Q in range(1, 401)
                                                        for c in (0, 1)}
    for PT, nct, Q, curl, pt, S, res, aff, launch_curved, launch_affine in plans:
        key = (PT, nct, Q, curl)
        assert pt == PT and S == dc.stride(PT), key
        assert bool(res) == dc.resident_fits(PT, nct, Q, bool(curl)), key
        assert bool(aff) == dc.affine_fits(PT, nct, Q, bool(curl)), key
        # what a launch asks for: the fit test's bytes (tables + the exchange of the curved form's 8 waves) and the weight prefix
        prefix = 8 * (((Q + 3) // 4 * 4 + 31) // 32 * 32)
        assert launch_curved == dc.lds_bytes(PT, nct, Q, bool(curl)) + prefix, key
        assert launch_affine == launch_curved + (8 * (dc.WAVES["affine"] - dc.WAVES["curved"]) * 4 * PT * 64 if curl else 0), key
        # a block that is given a form can be launched in it
        if res:
            assert launch_curved <= 160 * 1024, key
        assert bool(aff) == (PT <= 3 and Q > 1 and launch_affine <= 160 * 1024), key


def test_list_rule_agrees_with_geometry_form(sweep):
    lists = {(int(l[1]), int(l[2])): bool(int(l[3])) for l in sweep if l[0] == "lists"}
    assert set(lists) == {(na, nb) for nb in range(1, 41) for na in range(nb + 1)}
    for (na, nb), use in lists.items():
        J = np.ones((dc.KEB * nb, 2, 1, 1))
        J[dc.KEB * na:, 1] = 2.0  # the blocks behind the first `na`: a Jacobian that varies with the point
        form, (n_aff, n_curved) = dc.geometry_form(J)
        assert (n_aff, n_curved) == (na, nb - na)
        assert use == (form == "list"), (na, nb, form)


def test_host_check_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, run once on its own."""
    exe = str(tmp_path / "dense_host_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + INC, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
