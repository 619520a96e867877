"""Time the evaluation phase: the metrics launch, ``evaluate()`` and the reference-style loop.

    python tools/eval_time.py [--batch 64] [--clips 512] [--reps 30] [--epochs 3]
                              [--out profiles/eval/eval_time.json]

On a synthetic on-disk dataset of NTU shape ``(clips, 3, 300, 25, 2)``, 60 classes (written
to a temporary directory), with one ``Model`` in eval mode:
* ``kernel``: event-timed ``sgcn_score_metrics`` + ``sgcn_batch_loss`` on one batch of
  ``(batch, 60)`` float32 logits (``ScoreMetrics.update``), and ``sgcn_score_metrics`` alone
  on a whole 4-stream score set ``(4, 16384, 60)`` (``fuse_scores``' launch); median / min /
  max over --reps after a warm-up;
* ``evaluate``: wall time of ``shiftgcn.evaluate`` over the dataset (result() included);
* ``host_loop``: wall time of the loop of main.py:450-515 on the same model and loader: per
  batch the forward, torch's CrossEntropy, ``.cpu()`` of logits and loss and ``torch.max``
  for the prediction; then ``Feeder.top_k`` (the host argsort) for k = 1 and 5;
both alternating, --epochs passes each after one warm-up pass. One JSON line, also written to
--out. A report, not a gate. Needs a GPU: there is no CPU fallback for the launches.
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "shift-gcn_amd"))

import shiftgcn  # noqa: E402
from shiftgcn.evaluate import ScoreMetrics, score_metrics  # noqa: E402
from shiftgcn.feeder import DeviceBatchLoader, Feeder  # noqa: E402

T, V, M, C = 300, 25, 2, 60


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def write_dataset(path, n):
    rng = np.random.default_rng(0)
    data = np.lib.format.open_memmap(os.path.join(path, "data.npy"), mode="w+",
                                     dtype=np.float32, shape=(n, 3, T, V, M))
    for i in range(0, n, 64):
        data[i:i + 64] = rng.standard_normal(data[i:i + 64].shape, dtype=np.float32)
    data.flush()
    with open(os.path.join(path, "label.pkl"), "wb") as f:
        pickle.dump(([f"clip{i:06d}" for i in range(n)],
                     [int(v) for v in rng.integers(0, C, n)]), f)
    return os.path.join(path, "data.npy"), os.path.join(path, "label.pkl")


def host_loop(model, loader):
    """main.py:450-515 without the file writes."""
    loss_value, score_frag, predicted = [], [], []
    for data, label, _ in loader:
        with torch.no_grad():
            output = model(data)
            loss = torch.nn.functional.cross_entropy(output, label)
        score_frag.append(output.cpu().numpy())
        loss_value.append(loss.cpu().numpy())
        _, predict_label = torch.max(output, 1)
        predicted.append(predict_label.cpu().numpy())
    score = np.concatenate(score_frag)
    return {"mean_loss": float(np.mean(loss_value)),
            "topk": {k: loader.feeder.top_k(score, k) for k in (1, 5)}}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval", "eval_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_time needs a GPU")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "clips": a.clips,
           "shape": [a.clips, 3, T, V, M], "num_class": C}
    # the launches alone
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(a.batch, C, generator=g).to(dev)
    labels = torch.randint(0, C, (a.batch,), generator=g).to(dev)
    sm = ScoreMetrics(C, capacity=a.batch, device=dev)

    def one_update():
        sm.reset()
        sm.update(logits, labels)
    big = torch.randn(4, 16384, C, generator=g).to(dev)
    big_y = torch.randint(0, C, (16384,), generator=g).to(dev)
    fused = torch.empty(16384, C, device=dev)
    work = torch.empty(2, 16384, device=dev, dtype=torch.float64)
    hits = torch.zeros(2, device=dev, dtype=torch.int32)
    conf = torch.zeros(C * C, device=dev, dtype=torch.int32)
    res["kernel"] = {
        "update_batch": timed(one_update, a.reps),
        "counter_fill_alone": timed(sm.reset, a.reps),
        "fuse_4x16384": timed(lambda: score_metrics(
            big, big_y, (0.6, 0.6, 0.4, 0.4), (1, 5), 0, fused, work[0], work[1], None, None,
            hits, conf, None), a.reps),
        "torch_cross_entropy_batch": timed(
            lambda: torch.nn.functional.cross_entropy(logits, labels), a.reps),
    }
    with tempfile.TemporaryDirectory() as tmp:
        dp, lp = write_dataset(tmp, a.clips)
        fd = Feeder(dp, lp)
        model = shiftgcn.Model(num_class=C, num_point=V, num_person=M,
                               graph="graph.ntu_rgb_d.Graph").to(dev).eval()
        arms = {"evaluate": lambda: shiftgcn.evaluate(
                    model, DeviceBatchLoader(fd, a.batch, shuffle=False)),
                "host_loop": lambda: host_loop(model, DeviceBatchLoader(fd, a.batch,
                                                                        shuffle=False))}
        out = {}
        for name, fn in arms.items():       # warm-up: page cache, pinned buffers, eval caches
            out[name] = wall(fn)[1]
        ms = {name: [] for name in arms}
        for _ in range(a.epochs):
            for name, fn in arms.items():
                ms[name].append(wall(fn)[0])
        for name in arms:
            res[name] = {"ms": ms[name], "median_ms": float(np.median(ms[name])),
                         "batches": -(-a.clips // a.batch)}
        res["agreement"] = {
            "top1": [out["evaluate"]["topk"][1], out["host_loop"]["topk"][1]],
            "top5": [out["evaluate"]["topk"][5], out["host_loop"]["topk"][5]],
            "mean_loss": [out["evaluate"]["mean_loss"], out["host_loop"]["mean_loss"]]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
