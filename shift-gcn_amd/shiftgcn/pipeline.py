"""A whole landmark sequence scored on the device (the product chain of
``inference_pipeline.py``): sliding windows, skeleton pre-normalisation, the four-stream
ensemble, per-frame scores and fall intervals.

Reference: ``inference_pipeline.py:252-281`` (``create_sliding_windows``), ``:167-245``
(``pre_normalize``, the training-time ``data_gen/preprocess.py:8-91`` with the MediaPipe
joints), ``:377-386`` (``aggregate_per_frame``) and ``:389-424`` (``detect_fall_intervals``).

The reference cuts, pads and normalises every window on the host in a Python loop over
window x person x frame, runs the models window by window and averages in numpy. Here the
sequence goes up once, ``sgcn_window_normalize`` produces every pre-normalised window in
one launch in the layout :class:`shiftgcn.ensemble.Ensemble` takes, the windows run through
the ensemble in batches (one reused hipGraph), and ``sgcn_window_aggregate`` averages the
scores per frame. The only host step is the window table, a handful of integers.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .ensemble import EnsembleGraph

# pre_normalization's zaxis = [bottom, top], xaxis = [right, left], center_joint (one joint
# or the mean of two)
Skeleton = namedtuple("Skeleton", "zaxis xaxis center")
MEDIAPIPE = Skeleton((23, 11), (12, 11), (23, 24))   # inference_pipeline.py:140
NTU = Skeleton((0, 1), (8, 4), (1,))                 # data_gen/preprocess.py:8


def sliding_window_table(T, window_size=300, stride=150):
    """The windows of ``create_sliding_windows`` as int32 ``(n, 2)`` rows {start, num_real}:
    one window when ``T <= window_size``, else a window every ``stride`` frames up to and
    including the first that reaches the end (the last may be partial)."""
    if T <= 0 or window_size <= 0 or stride <= 0:
        raise ValueError("T, window_size and stride must be positive")
    if T <= window_size:
        return np.array([[0, T]], dtype=np.int32)
    n = -(-(T - window_size) // stride) + 1          # first start with start + window >= T
    start = np.arange(n, dtype=np.int64) * stride
    start = start[start < T]                         # (a stride beyond the window can skip the end)
    return np.stack([start, np.minimum(start + window_size, T) - start], 1).astype(np.int32)


def check_table(table, window_size=None, total_frames=None):
    """A host window table as contiguous int32 ``(n, 2)``; ValueError for a row that is
    negative, longer than the window or past the end of the sequence."""
    table = np.ascontiguousarray(table, dtype=np.int32)
    if table.ndim != 2 or table.shape[1] != 2:
        raise ValueError("table must be (n, 2) rows of {start, num_real}")
    start, real = table[:, 0].astype(np.int64), table[:, 1].astype(np.int64)
    if (start < 0).any() or (real < 0).any():
        raise ValueError("table: negative start or num_real")
    if window_size is not None and (real > window_size).any():
        raise ValueError("table: num_real exceeds the window size")
    if total_frames is not None and (start + real > total_frames).any():
        raise ValueError("table: a window ends past the sequence")
    return table


def _device_table(table, device, window_size=None, total_frames=None):
    """The table on the device; a host table is checked first (the kernels clamp a device
    table's rows, they cannot reject them)."""
    if isinstance(table, torch.Tensor):
        if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 2 \
                or not table.is_contiguous() or table.device != device:
            raise ValueError("table must be a contiguous int32 (n, 2) tensor on the device")
        return table
    return torch.from_numpy(check_table(table, window_size, total_frames)).to(device)


def normalize_windows(seq, table, window_size, skeleton=MEDIAPIPE, stages=7, out=None):
    """Every window of ``seq`` ``(3, T, V, M)`` listed in ``table`` (host int32 ``(n, 2)``
    or the same on the device), zero-padded to ``window_size`` and pre-normalised as
    ``pre_normalize`` does: ``(n, 3, window_size, V, M)`` on the device, one launch.

    ``stages`` selects a prefix of the chain (1 pad, 2 centre, 4 rotate; 7 = all of it)."""
    ops.check_input(seq, "seq")
    if seq.dim() != 4 or seq.shape[0] != 3:
        raise ValueError("seq must be (3, T, V, M)")
    _, T, V, M = seq.shape
    table = _device_table(table, seq.device, window_size, T)
    n = table.shape[0]
    shape = (n, 3, window_size, V, M)
    if out is None:
        out = torch.empty(shape, device=seq.device, dtype=torch.float32)
    else:
        ops.check_input(out, "out")
        if tuple(out.shape) != shape or out.device != seq.device:
            raise ValueError(f"out must be {shape} on the sequence's device")
    center = tuple(skeleton.center)
    if len(center) not in (1, 2):
        raise ValueError("the centre is one joint or the mean of two")
    with ops._timed("window_normalize", 0, 4 * (seq.numel() + out.numel()), seq):
        rc = _lib.load().sgcn_window_normalize(
            seq.data_ptr(), table.data_ptr(), out.data_ptr(), n, T, V, M, window_size,
            skeleton.zaxis[0], skeleton.zaxis[1], skeleton.xaxis[0], skeleton.xaxis[1],
            center[0], center[1] if len(center) == 2 else -1, int(stages), ops._stream(seq))
    _lib.check(rc, "sgcn_window_normalize")
    return out


def aggregate_per_frame(scores, table, total_frames):
    """``aggregate_per_frame`` on the device: the float64 mean, per frame, of the scores of
    the windows whose real frames cover it (0 where none does)."""
    ops.check_input(scores, "scores", torch.float64)
    table = _device_table(table, scores.device, None, total_frames)
    if scores.dim() != 1 or scores.shape[0] != table.shape[0]:
        raise ValueError("one score per table row")
    per_frame = torch.empty(total_frames, device=scores.device, dtype=torch.float64)
    with ops._timed("window_aggregate", 0, 8 * (scores.numel() + total_frames), scores):
        rc = _lib.load().sgcn_window_aggregate(
            scores.data_ptr(), table.data_ptr(), per_frame.data_ptr(), table.shape[0],
            total_frames, ops._stream(scores))
    _lib.check(rc, "sgcn_window_aggregate")
    return per_frame


def _clock(frame, fps):
    minutes, rest = divmod(frame / fps, 60.0)
    return f"{int(minutes)}:{rest:05.2f}"


def detect_fall_intervals(per_frame, threshold, fps):
    """Host side: the maximal runs of frames whose score exceeds ``threshold``, as the
    reference's detection dicts (frames, ``m:ss.ss`` times, mean / peak confidence)."""
    if isinstance(per_frame, torch.Tensor):
        per_frame = per_frame.detach().cpu().numpy()
    per_frame = np.asarray(per_frame)
    above = np.zeros(len(per_frame) + 2, dtype=np.int8)
    above[1:-1] = per_frame > threshold
    step = np.diff(above)
    found = []
    for s, e in zip(np.flatnonzero(step > 0), np.flatnonzero(step < 0)):
        region = per_frame[s:e]
        found.append({
            "start_frame": int(s),
            "end_frame": int(e),
            "start_time": _clock(int(s), fps),
            "end_time": _clock(int(e), fps),
            "mean_confidence": float(np.mean(region)),
            "peak_confidence": float(np.max(region)),
            "peak_frame": int(s + int(np.argmax(region))),
        })
    return found


class SequenceScorer:
    """``score(world)``: per-frame fall scores of a landmark sequence ``(3, T, V, M)``
    (numpy or device tensor): one normalise launch for all windows, the ensemble over the
    windows in chunks of ``batch``, one aggregate launch.

    Every chunk holds ``batch`` windows (the last is padded with zero windows whose scores
    are dropped; so is a sequence with fewer windows than ``batch``), so with ``graph=True``
    every chunk of every sequence replays the one :class:`EnsembleGraph` the scorer holds.
    Returns ``(per_frame, window_scores,
    table)``: two float64 device tensors and the host window table; nothing is copied back
    unless the caller reads it."""

    def __init__(self, ensemble, window_size=300, stride=150, batch=16, graph=True,
                 skeleton=MEDIAPIPE):
        if batch <= 0:
            raise ValueError("batch must be positive")
        self.ensemble = ensemble
        self.window_size, self.stride, self.batch = int(window_size), int(stride), int(batch)
        self.graph = bool(graph)
        self.skeleton = skeleton
        self._graph = None

    def _run(self, chunk):
        if not self.graph:
            return self.ensemble(chunk)[0]
        if self._graph is None or self._graph.static_in.shape != chunk.shape:
            self._graph = EnsembleGraph(self.ensemble, chunk.shape, chunk.device)
        return self._graph.run(chunk)[0]

    @torch.no_grad()
    def score(self, world):
        device = self.ensemble.parent.device
        if not isinstance(world, torch.Tensor):
            world = torch.from_numpy(np.ascontiguousarray(world, dtype=np.float32))
        seq = world.to(device=device, dtype=torch.float32).contiguous()
        if seq.dim() != 4 or seq.shape[0] != 3:
            raise ValueError("world must be (3, T, V, M)")
        _, T, V, M = seq.shape
        table = sliding_window_table(T, self.window_size, self.stride)
        n = len(table)
        bs = self.batch
        padded = -(-n // bs) * bs
        table_d = torch.from_numpy(table).to(device)
        wins = torch.empty((padded, 3, self.window_size, V, M), device=device,
                           dtype=torch.float32)
        wins[n:].zero_()
        normalize_windows(seq, table_d, self.window_size, self.skeleton, out=wins[:n])
        scores = torch.empty(padded, device=device, dtype=torch.float64)
        for i in range(0, padded, bs):
            scores[i:i + bs].copy_(self._run(wins[i:i + bs]))
        window_scores = scores[:n]
        return aggregate_per_frame(window_scores, table_d, T), window_scores, table
