"""Time the device augmentation (sgcn_clip_augment) and the DeviceBatchLoader with and
without it.

    python tools/augment_time.py [--batch 64] [--clips 1024] [--reps 30] [--epochs 3]

One JSON line:
* ``kernel``: event-timed ``sgcn_clip_augment`` at the NTU batch ``(batch, 3, 300, 25, 2)``
  with every flag on (normalization, random_shift, random_choose at window 300 so that
  T_out = T, random_move), next to a ``torch`` device copy of the same tensor (the
  read-once / write-once yardstick); median / min / max over --reps after a warm-up.
* ``host``: per-batch host time of the two steps that stay on the host, the extents
  (``ClipAugment.batch_extents``) and the draws (``ClipAugment.draw`` + ``pack``).
* ``loader``: batches/s of one epoch of ``DeviceBatchLoader`` over a synthetic on-disk NTU
  dataset (the format of tools/make_clip_dataset.py, --clips clips, written to a temporary
  directory), with and without ``augment``, alternating, --epochs epochs each after one
  warm-up epoch; the consumer only waits for each batch.
Needs a GPU: there is no CPU fallback for the launch.
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

from shiftgcn.augment import AugmentedFeeder, ClipAugment  # noqa: E402
from shiftgcn.feeder import DeviceBatchLoader, Feeder  # noqa: E402

T, V, M = 300, 25, 2


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
        blk = rng.standard_normal(data[i:i + 64].shape, dtype=np.float32)
        for j in range(len(blk)):          # NTU clips end in zero frames (short actions)
            blk[j, :, T - int(rng.integers(0, 200)):] = 0
        data[i:i + 64] = blk
    data.flush()
    with open(os.path.join(path, "label.pkl"), "wb") as f:
        pickle.dump(([f"clip{i:06d}" for i in range(n)],
                     [int(v) for v in rng.integers(0, 60, n)]), f)
    return os.path.join(path, "data.npy"), os.path.join(path, "label.pkl")


def epoch_rate(loader):
    t0 = time.perf_counter()
    n = 0
    for x, y, _ in loader:
        n += 1
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time needs a GPU")
    spec = dict(random_choose=True, random_shift=True, random_move=True, window_size=T,
                normalization=True)
    res = {"batch": a.batch, "shape": [a.batch, 3, T, V, M]}
    with tempfile.TemporaryDirectory() as tmp:
        dp, lp = write_dataset(tmp, a.clips)
        fd = AugmentedFeeder(dp, lp, seed=0, **spec)
        aug = fd.augment
        raw = np.array(fd.data[:a.batch])
        # the two host steps
        host = {"extents_ms": [], "draw_ms": []}
        for _ in range(10):
            t0 = time.perf_counter()
            ext = aug.batch_extents(raw)
            t1 = time.perf_counter()
            p = aug.draw(ext, T)
            p.pack()
            t2 = time.perf_counter()
            host["extents_ms"].append(1e3 * (t1 - t0))
            host["draw_ms"].append(1e3 * (t2 - t1))
        res["host"] = {k: float(np.median(v)) for k, v in host.items()}
        # the launch next to a device copy of the same tensor
        x = torch.from_numpy(raw).cuda()
        out = torch.empty_like(x)
        p.device_buf = torch.from_numpy(p.pack()).cuda()
        nbytes = 2 * x.numel() * 4
        k = timed(lambda: aug.apply_device(x, p, out=out), a.reps)
        c = timed(lambda: out.copy_(x), a.reps)
        for r in (k, c):
            r["GBps_at_median"] = nbytes / r["median_ms"] / 1e6
        res["kernel"] = {"clip_augment": k, "torch_copy": c, "bytes": nbytes}
        # one epoch of the loader with and without the augmentation
        plain = Feeder(dp, lp)
        mk = {"augmented": lambda: DeviceBatchLoader(fd, a.batch, shuffle=True, drop_last=True),
              "plain": lambda: DeviceBatchLoader(plain, a.batch, shuffle=True, drop_last=True)}
        rates = {name: [] for name in mk}
        for name in mk:
            epoch_rate(mk[name]())                    # warm-up (page cache, pinned buffers)
        for _ in range(a.epochs):
            for name in mk:
                rates[name].append(epoch_rate(mk[name]()))
        res["loader"] = {name: {"batches_per_s": v, "median": float(np.median(v)),
                                "clips_per_s_median": float(np.median(v)) * a.batch}
                         for name, v in rates.items()}
        res["loader"]["batches_per_epoch"] = a.clips // a.batch
    print(json.dumps(res))


if __name__ == "__main__":
    main()
