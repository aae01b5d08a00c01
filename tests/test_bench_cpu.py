"""bench.py host logic that needs no GPU: the roofline `traffic` lookup."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_headline_traffic_is_attached_to_the_chain_schedule():
    t = bench.load_traffic("rq1.botnet.static")
    assert set(t) >= {"k_mlp", "k_survive"}
    assert {"k_genc"} <= set(t) or {"k_gen", "k_cons"} <= set(t)
    assert all(v > 0 for v in t.values())


def test_unmeasured_workload_gets_no_traffic():
    assert bench.load_traffic("synthetic.botnet.wide") == {}


def test_dump_outputs_writes_a_fixed_sample_of_whole_states(tmp_path, monkeypatch):
    """--dump-outputs: every state below the size cap; above it the same seeded sample of
    whole states on every call, named in state_index.npy; float64 files."""
    import numpy as np
    import torch

    rng = np.random.default_rng(3)
    genes = torch.from_numpy(rng.standard_normal((7, 5, 4)))
    F = torch.from_numpy(rng.standard_normal((7, 5, 3)))
    bench.dump_outputs(str(tmp_path / "all"), genes, F)
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "genes.npy"), genes.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "F.npy"), F.numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "state_index.npy"), np.arange(7.0))
    # a cap of three states (7 x 5 x (4 + 3) fp64 = 280 bytes per state)
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 280 + 279)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), genes, F)
    idx = np.load(tmp_path / "a" / "state_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (3,)
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 7
    sel = idx.astype(int)
    for name, full in (("genes.npy", genes), ("F.npy", F), ("state_index.npy", None)):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, b)
        if full is not None:
            np.testing.assert_array_equal(a, full.numpy()[sel])
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) \
        < 3 * 280 + 279 + 3 * 8 + 3 * 128  # the arrays plus three .npy headers
