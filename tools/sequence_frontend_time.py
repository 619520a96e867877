"""Time the sequence front end (sgcn_window_normalize, sgcn_window_aggregate) on the GPU
next to the numpy closed form of tests/pipeline_oracle.py on the host.

    python tools/sequence_frontend_time.py [--frames 18000] [--window 300] [--stride 150]
                                           [--reps 20] [--cpu 1]

A synthetic MediaPipe sequence (seeded; a few null runs) -> one JSON line: the event-timed
median / min / max of each launch over --reps repetitions after a warm-up (and the mean of
the same launches issued back to back), and the host
time of the same normalisation and aggregation in numpy. Needs a GPU: there is no CPU
fallback for the launches.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "shift-gcn_amd"), os.path.join(REPO, "tests"),
          os.path.join(REPO, "tests", "golden")):
    sys.path.insert(0, p)

import formula  # noqa: E402
import pipeline_oracle as po  # noqa: E402
from shiftgcn import pipeline  # noqa: E402


def sequence(T):
    pose = formula.tensor((3, 1, 33, 1), 11, 1.0).numpy()
    seq = (pose + formula.tensor((3, T, 33, 1), 12, 0.25).numpy()).astype(np.float32)
    for a in range(500, T, 2500):            # null runs: leading, middle and trailing fills
        seq[:, a:a + 40] = 0.0
    return seq


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
    # and the same launches back to back inside one event pair (the queue never drains)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms),
            "back_to_back_ms": e0.elapsed_time(e1) / reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18000)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--stride", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu", type=int, default=1, help="also time the numpy closed form")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sequence_frontend_time needs a GPU")
    seq = sequence(a.frames)
    table = pipeline.sliding_window_table(a.frames, a.window, a.stride)
    d_seq = torch.from_numpy(seq).cuda()
    d_table = torch.from_numpy(table).cuda()
    out = torch.empty((len(table), 3, a.window, 33, 1), device="cuda")
    scores = (0.5 + torch.from_numpy(formula.hash_uniform(len(table), 13))).cuda()
    res = {"frames": a.frames, "window": a.window, "stride": a.stride, "windows": len(table),
           "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    res["normalize"] = timed(lambda: pipeline.normalize_windows(d_seq, d_table, a.window,
                                                                out=out), a.reps)
    res["aggregate"] = timed(lambda: pipeline.aggregate_per_frame(scores, d_table, a.frames),
                             a.reps)
    if a.cpu:
        t0 = time.perf_counter()
        want = po.normalize_windows(seq, table, a.window)
        t1 = time.perf_counter()
        agg = po.aggregate_per_frame(scores.cpu().numpy(), table, a.frames)
        t2 = time.perf_counter()
        res["numpy_normalize_ms"] = 1e3 * (t1 - t0)
        res["numpy_aggregate_ms"] = 1e3 * (t2 - t1)
        got = out.cpu().numpy()
        res["max_abs_diff_vs_numpy"] = float(np.abs(got - want).max())
        res["aggregate_equal"] = bool(np.array_equal(
            pipeline.aggregate_per_frame(scores, d_table, a.frames).cpu().numpy(), agg))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
