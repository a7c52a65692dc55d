"""Shared by tests/test_transient_host.py and tests/test_transient_gpu.py: the reference's coaxial transient example from the
committed fixture (tests/golden/coaxial_matched.npz, written by tests/golden/make_coaxial_golden.py) and its run through the CPU
restatement, computed once per process."""
import functools
import os

import numpy as np

from palace_amd.fem import transient as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coaxial_matched.npz")
COLUMNS = tr.TransientReferenceSystem.COLUMNS


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def coaxial_mesh():
    from palace_amd.fem.mesh import HexMesh

    d = golden()
    return HexMesh(d["x"], d["elem_nodes"].astype(np.int64), d["attr"], d["bdr_faces"].astype(np.int64), d["bdr_attr"])


@functools.lru_cache(maxsize=None)
def coaxial_reference_run():
    """(system, {column: [201]}): coaxial_matched through reference_steps (about a quarter of a minute of CPU time)."""
    system = tr.TransientReferenceSystem(None, coaxial_mesh())
    return system, system.run_reference()


def check_against_golden(series, label):
    """Every entry of every column under the reference's own rule (rtol 2e-2, atol 1e-11); the energies, which that rule passes
    vacuously (1e-20 J against atol 1e-11), also to 2e-2 of their column's peak.  Returns the worst deviation per column relative
    to the column's peak."""
    d = golden()
    assert np.allclose(series["t_ns"], d["t_ns"], rtol=0.0, atol=1e-12)
    worst = {}
    for k in COLUMNS:
        got, want = series[k], d[k]
        assert got.shape == want.shape == (201,)
        peak = np.abs(want).max()
        worst[k] = np.abs(got - want).max() / peak
        print(f"{label} {k}: worst deviation {worst[k]:.2e} of the peak {peak:.3e}")
    for k in COLUMNS:
        ok = tr.regression_close(series[k], d[k])
        assert ok.all(), (k, np.nonzero(~ok)[0][:10])
    for k in ("E_elec", "E_mag"):
        assert worst[k] <= 2.0e-2, (k, worst[k])
    return worst
