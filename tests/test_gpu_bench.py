"""bench.py's plain run on the GPU: the result line holds the headline figure and
ms_per_step for exactly --steps timed steps, nothing that only --full measures, and
--dump-outputs writes the last step's final populations, identical from run to run."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, ROOT)

FULL_ONLY = {"roofline", "kernels", "kernels_avg_ms_per_generation", "kernel_times_generations",
             "generate", "cpu_baseline", "configs"}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def plain_run(monkeypatch, capsys, steps, warmup, out):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps),
                                      "--warmup", str(warmup), "--workload",
                                      "rq1.botnet.static.48", "--n-gen", "4",
                                      "--dump-outputs", str(out)])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1  # one JSON result line on stdout
    return json.loads(lines[0])


def test_plain_run_line_and_reproducible_dump(monkeypatch, capsys, tmp_path):
    r1 = plain_run(monkeypatch, capsys, 1, 0, tmp_path / "a")
    r2 = plain_run(monkeypatch, capsys, 3, 1, tmp_path / "b")
    for r, steps in ((r1, 1), (r2, 3)):
        assert r["steps"] == steps and r["unit"] == "evals/s" and r["dtype"] == "f64"
        assert r["higher_is_better"] is True and r["ms_per_step"] > 0
        assert not FULL_ONLY & set(r)
        # value and ms_per_step describe the same timed steps: 48 states x (P + 3 * O) evals
        evals = 48 * (203 + 3 * 100)
        assert r["value"] == pytest.approx(evals / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert sorted(os.listdir(tmp_path / "a")) == ["F.npy", "genes.npy", "state_index.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    b = {n: np.load(tmp_path / "b" / n) for n in os.listdir(tmp_path / "b")}
    assert a["genes.npy"].shape[:2] == (48, 203) and a["F.npy"].shape == (48, 203, 3)
    np.testing.assert_array_equal(a["state_index.npy"], np.arange(48.0))
    for n in a:
        assert a[n].dtype == np.float64 and np.isfinite(a[n]).all()
        np.testing.assert_array_equal(a[n], b[n])
