"""The flux error estimators at order 5 through the C++ front end (palace_amd/csrc/errorestimator.hpp on the six-point kernels
of pa_rt_hex_q6.hip and pa_mixed_hex_q6.hip): examples/cxx_host/estimate_hex.cpp and estimate_hex_mg.cpp with the criteria of
tests/test_cxx_estimator_hex_gpu.py and tests/test_cxx_estimator_hex_mg_gpu.py.  The multigrid run builds the Raviart-Thomas
hierarchy on the pairs (1 ... 5, 6), assembles its (1, 6) level in full and runs the ComplexVector estimators on two one-part
passes (no both-parts-per-pass kernel at six points)."""
import re
import subprocess

import numpy as np
import pytest

from tests.test_cxx_estimator_hex_gpu import exe as exe_hex  # noqa: F401  (fixtures: the built examples)
from tests.test_cxx_estimator_hex_mg_gpu import KINDS, _line
from tests.test_cxx_estimator_hex_mg_gpu import exe as exe_mg  # noqa: F401

pytestmark = pytest.mark.gpu
P = 5


def test_cxx_hex_estimators_at_order_five(exe_hex):
    import dump_estimator_hex_problem as dp
    from tests.test_mixed_hex_gpu import device_estimate

    binary, d = exe_hex
    blob, out = str(d / f"problem{P}.bin"), str(d / f"est{P}.bin")
    dp.main(blob, P)
    r = subprocess.run([binary, blob, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    prob = dp.problem(P)
    ne, nrt, nnd = prob["mesh"].ne, prob["rt"].ndofs, prob["nd"].ndofs
    got = np.fromfile(out, dtype=np.float64)
    assert got.size == 3 * ne + nrt + nnd
    eg, ec, both, D, H = np.split(got, [ne, 2 * ne, 3 * ne, 3 * ne + nrt])
    for name, est, flux, field, mats in (("grad", eg, D, prob["E"], prob["eps"]), ("curl", ec, H, prob["B"], prob["muinv"])):
        est_p, flux_p, its_p = device_estimate(prob["mesh"], P, name, field, mats)
        ee, ef = np.abs(est - est_p).max() / est_p.max(), np.abs(flux - flux_p).max() / np.abs(flux_p).max()
        its = int(re.search(name + r": pcg_its (\d+)", r.stdout).group(1))
        print(f"{name}: estimates {ee:.2e} smooth flux {ef:.2e} iterations {its} / {its_p}")
        assert ee < 1e-9 and ef < 1e-9 and est_p.min() > 0
        assert abs(its - its_p) <= 1
    assert np.abs(both - np.sqrt(eg + ec)).max() < 1e-12 * both.max()


def test_cxx_estimators_with_multigrid_projectors_at_order_five(exe_mg):
    import dump_estimator_hex_mg_problem as dp

    binary, d = exe_mg
    blob, out = str(d / f"problem{P}.bin"), str(d / f"est{P}.bin")
    dp.main(blob, P)
    r = subprocess.run([binary, blob, out, "1e-12"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    print(r.stdout)
    ne = int(re.search(r"hexes (\d+) order", r.stdout).group(1))
    est = np.fromfile(out, dtype=np.float64).reshape(3, 4, ne)
    jac, mg, amg = _line(r.stdout, "jacobi"), _line(r.stdout, "mg"), _line(r.stdout, "amg")
    assert "all_converged 1" in r.stdout
    for run in (jac, mg, amg):
        assert run["converged"] == [1, 1, 1, 1], run
    assert (jac["levels"], mg["levels"], amg["levels"]) == (1, P, 1)
    assert jac["use_mg"] == [0, 0, 0, 0] and mg["use_mg"] == [1, 1, 1, 1] and amg["use_mg"] == [1, 1, 1, 1]
    assert np.isfinite(est).all() and (est[0] > 0.0).all()
    for k, kind in enumerate(KINDS):
        scale = est[0, k].max()
        d_mg, d_amg = np.abs(est[1, k] - est[0, k]).max() / scale, np.abs(est[2, k] - est[0, k]).max() / scale
        print(f"{kind}: |mg - jacobi| {d_mg:.2e} |amg - jacobi| {d_amg:.2e} of the largest estimate")
        assert d_mg <= 1e-8
        assert d_amg <= 1e-8
    # strictly fewer iterations with the multigrid cycle
    print("iterations with the cycle / with Jacobi:", mg["its"], jac["its"])
    for kind in KINDS:
        assert 0 < mg["its"][kind] < jac["its"][kind], (kind, mg["its"], jac["its"])
