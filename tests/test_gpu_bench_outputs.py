"""bench.py on the GPU, in this process (tiny batches): what a plain run's line holds and what
``--dump-outputs`` writes, for the training step and for the ensemble."""
import json
import sys

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with torch.random.fork_rng(devices=[0]):      # bench seeds the global generators
        bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {p.name[:-4]: np.load(p, allow_pickle=False) for p in d.iterdir()}


def test_plain_training_line_and_outputs(tmp_path, monkeypatch, capsys):
    """One timed step from the seeded initial weights on a seeded batch of 2 clips, twice.
    The line carries no roofline / CPU baseline leg; the dump holds the loss, and every
    parameter with its gradient and every buffer after the step, in float32 (the step
    counters, integers on the device, in float64). Both runs start from the same inputs, so
    the forward loss agrees to float32 summation-order error: 1e-4 relative covers ten
    blocks of contractions over K <= 256 terms each at eps = 6e-8 (10 * 256 * 6e-8 = 1.5e-4
    worst case, sqrt(K) growth in practice)."""
    runs = []
    for name in ("a", "b"):
        d = _run(monkeypatch, capsys, "--gpus", "1", "--steps", "1", "--warmup", "0",
                 "--batch", "2", "--dump-outputs", str(tmp_path / name))
        assert d["roofline"] is None and d["cpu_baseline"] is None
        assert d["steps"] == 1 and d["warmup"] == 0 and d["dtype"] == "fp32"
        assert d["ms_per_step"] > 0 and d["unit"] == "clips/s" and d["higher_is_better"]
        assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) <= 0.01 * d["value"]
        runs.append(_load(tmp_path / name))
    a, b = runs
    assert sorted(a) == sorted(b)
    assert a["loss"].shape == (1,) and a["loss"].dtype == np.float32
    print("loss", a["loss"], b["loss"])
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 1e-4 * abs(float(a["loss"][0]))
    assert a["param.fc.weight"].shape == (60, 256) == a["grad.fc.weight"].shape
    params = [k for k in a if k.startswith("param.")]
    assert sum(a[k].size for k in params) >= 693_107       # (the trainable ones alone)
    assert any(k.startswith("buffer.") and k.endswith("running_mean") for k in a)
    for k, v in a.items():
        assert np.all(np.isfinite(v)), k
        counter = k.endswith("num_batches_tracked")
        integer = counter or k.endswith((".shift_in", ".shift_out"))   # int64 on the device
        assert v.dtype == (np.float64 if integer else np.float32), k
        if counter:
            assert float(v) in (0.0, 1.0), k                # one step was run in all
    assert any(float(v) == 1.0 for k, v in a.items() if k.endswith("num_batches_tracked"))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    # the step moved the weights: the dump is the model after it, not the seeded start
    assert float(np.abs(a["grad.fc.weight"]).max()) > 0


def test_plain_ensemble_line_and_outputs(tmp_path, monkeypatch, capsys):
    d = _run(monkeypatch, capsys, "--gpus", "1", "--steps", "2", "--warmup", "1", "--config",
             "ens", "--batch", "2", "--dump-outputs", str(tmp_path))
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert d["steps"] == 2 and d["unit"] == "windows/s" and d["ms_per_step"] > 0
    out = _load(tmp_path)
    assert sorted(out) == ["logits", "scores"]
    s, lg = out["scores"], out["logits"]
    assert s.dtype == lg.dtype == np.float64 and s.shape == (2,) and lg.shape == (2, 2)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    assert np.allclose(s, e[:, 1] / e.sum(axis=1), rtol=1e-12, atol=0)
