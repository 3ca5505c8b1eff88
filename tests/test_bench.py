"""bench.py's plain and ``--full`` runs and ``--dump-outputs``.

A plain run reports the headline figures only; ``--full`` adds the roofline block and the parity spot check.
With the same arguments two runs feed the timed steps the same inputs and ProbSparse draws (the sampler chains
are reseeded after the clock-driven warm-up), so what ``--dump-outputs`` writes is bitwise the same from run to
run, and the dumped NMSE sums are NMSE_Split of the dumped predictions (FullPrecision/metrics.py:26-30).
"""
import json

import numpy as np
import pytest
import torch

ARGS = ["--gpus", "1", "--steps", "5", "--warmup", "3", "--settle-s", "0.05"]


def _run(capsys, extra):
    import bench

    bench.main(ARGS + extra)
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from channelestimationtransformer_amd.dataset import make_batch
    from oracle.metrics_np import nmse_split as ref_split

    a = _run(capsys, ["--dump-outputs", str(tmp_path / "a")])
    b = _run(capsys, ["--dump-outputs", str(tmp_path / "b"), "--full", "--no-cpu-baseline"])
    for r in (a, b):
        assert r["steps"] == 5 and r["unit"] == "seq/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] / (512 * 1e3) - 1) < 1e-2
    assert "roofline" not in a and "parity_rel_nmse_vs_oracle" not in a and "cpu_baseline" not in a
    assert b["roofline"]["kernel_ms"] > 0 and b["parity_rel_nmse_vs_oracle"] < 1e-4 and "cpu_baseline" not in b
    outs = {}
    for d in "ab":
        out, sums = np.load(tmp_path / d / "out.npy"), np.load(tmp_path / d / "nmse_sums.npy")
        assert out.dtype == np.float32 and out.shape == (512, 5, 16) and np.isfinite(out).all()
        assert sums.dtype == np.float64 and sums.shape == (2, 5)
        outs[d] = (out, sums)
    np.testing.assert_array_equal(outs["a"][0], outs["b"][0])
    np.testing.assert_array_equal(outs["a"][1], outs["b"][1])
    # step 4 ran on lane 0 (4 mod 2), whose labels come from the lane's seeded batch
    lab = make_batch(512, snr=20.0, seed=1234)[2]
    out, sums = outs["a"]
    np.testing.assert_allclose(sums[0] / sums[1], ref_split(out, lab), rtol=1e-5)
    assert a["nmse_db"] == b["nmse_db"]


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    """CPU part of the dump: float32 / float64 on disk, and a fixed seeded row sample past the byte budget."""
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    big = np.arange(64 * 32, dtype=np.float32).reshape(64, 32)
    small = np.arange(10, dtype=np.int64).reshape(2, 5)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    s = np.load(tmp_path / "x" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    assert x.dtype == np.float32 and np.array_equal(x, y)
    assert x.nbytes + s.nbytes <= 4096 and 1 <= x.shape[0] < 64
    rows = (x[:, 0] / 32).astype(int)
    assert np.array_equal(x, big[rows]) and np.all(np.diff(rows) > 0)
