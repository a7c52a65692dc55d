"""bench.py --dump-outputs: what the timed path computed, as .npy files under a size cap; an output larger than its share of the cap
is cut to the same seeded sample of positions in every run, so that two builds compare output for output."""
import os

import numpy as np
import torch

import bench


def test_dump_caps_the_bytes_and_samples_the_same_positions(tmp_path):
    y = torch.arange(3000, dtype=torch.float64) * 0.5
    a = bench.dump_outputs(str(tmp_path / "a"), {"y": y}, 1000 * 8)
    b = bench.dump_outputs(str(tmp_path / "b"), {"y": y}, 1000 * 8)
    ya, yb = (np.load(os.path.join(d["dir"], "y.npy")) for d in (a, b))
    assert a["arrays"]["y"]["entries"] == 1000 and a["arrays"]["y"]["of"] == 3000 and a["arrays"]["y"]["sample"]
    assert ya.dtype == np.float64 and np.array_equal(ya, yb)
    pos = (ya * 2).astype(np.int64)  # (the value at position i is i / 2)
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < 3000
    # two arrays share the budget; one that fits is written whole
    c = bench.dump_outputs(str(tmp_path / "c"), {"y": y, "z": y[:400]}, 1000 * 8)
    assert c["arrays"]["y"]["entries"] == 500 and c["arrays"]["z"] == {"entries": 400, "of": 400, "dtype": "float64", "sample": None}
    assert np.array_equal(np.load(os.path.join(c["dir"], "z.npy")), y[:400].numpy())
    assert bench.DUMP_BYTES + 2 * 128 <= 64e6  # (data plus .npy headers)
