"""The evaluation phase on the device: loss, top-k, confusion matrix and score fusion.

Reference: ``main.py:450-515`` (``eval``: per batch a forward, ``CrossEntropyLoss``, a copy of
logits and loss to the host and ``torch.max`` for the wrong/result files; then a host
``argsort`` of the whole score matrix per ``k`` and the ``sample_name -> score`` pickle) and
``ensemble.py`` (the four streams' saved scores fused with ``alpha = [0.6, 0.6, 0.4, 0.4]``,
top-1 / top-5 counted in a Python loop).

Here a batch costs one ``sgcn_score_metrics`` launch (fusion, per-sample loss, prediction,
rank of the label, hit counters, confusion matrix) and one ``sgcn_batch_loss`` launch (the
batch mean in a fixed float64 tree); nothing is read back until :meth:`ScoreMetrics.result`,
which makes the run's one device-to-host copy. The closed forms are in
``include/shiftgcn.h`` and DESIGN.md §Evaluation. Ties: a sample is a top-k hit iff
``label in np.argsort(row, kind="stable")[-k:]``; :meth:`Feeder.top_k` sorts with numpy's
default (unstable) kind, so the two agree exactly on rows without ties.

* :class:`ScoreMetrics` — the device-side run state and its ``update`` / ``result``.
* :func:`evaluate` — a :class:`Model` in ``.eval()`` or an :class:`Ensemble` over a
  :class:`DeviceBatchLoader`; writes the reference's wrong / result / score files.
* :func:`fuse_scores` — ``ensemble.py`` for saved scores, in one launch.
* :func:`cross_entropy` — the mean loss as an autograd Function over the same kernels
  (``train.cross_entropy``).
There is no CPU path: scores on the host raise like every other wrapper.
"""
from __future__ import annotations

import ctypes
import pickle

import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream, _timed, check_input

_F64 = torch.float64
_I64 = torch.int64


def _check_labels(labels, n, device):
    if not labels.is_cuda or labels.device != device:
        raise RuntimeError("labels must be a CUDA tensor on the scores' device")
    if labels.dtype != _I64 or not labels.is_contiguous() or labels.shape != (n,):
        raise RuntimeError(f"labels must be a contiguous int64 ({n},) tensor")


def score_metrics(scores, labels, weights=None, topk=(), row_offset=0, fused=None, loss=None,
                  lse=None, pred=None, rank=None, hits=None, confusion=None, bad_labels=None):
    """``sgcn_score_metrics`` on ``scores`` (n, C), or (S, n, C) with S ``weights``; the
    outputs are rows ``row_offset + i`` of the given buffers (``loss``, ``lse``: float64,
    allocated when left out; the others optional). Returns ``(loss, lse)``."""
    if scores.dim() == 2:
        scores = scores.unsqueeze(0)
    if scores.dim() != 3:
        raise ValueError("scores must be (n, C) or (S, n, C)")
    if scores.dtype not in (torch.float32, _F64):
        raise RuntimeError(f"scores must be float32 or float64 (got {scores.dtype})")
    check_input(scores, "scores", scores.dtype)
    S, n, C = scores.shape
    if S > 1 and (weights is None or len(weights) != S):
        raise ValueError(f"{S} score streams need {S} weights")
    _check_labels(labels, n, scores.device)
    if loss is None:
        loss = torch.empty(row_offset + n, device=scores.device, dtype=_F64)
    if lse is None:
        lse = torch.empty(row_offset + n, device=scores.device, dtype=_F64)
    rows = row_offset + n
    for t, name, dt, per in ((fused, "fused", scores.dtype, C), (loss, "loss", _F64, 1),
                             (lse, "lse", _F64, 1), (pred, "pred", torch.int32, 1),
                             (rank, "rank", torch.int32, 1)):
        if t is not None:
            check_input(t, name, dt)
            if t.numel() < rows * per:
                raise ValueError(f"{name} holds fewer than {rows} rows")
    topk = [int(k) for k in topk]
    if topk:
        check_input(hits, "hits", torch.int32)
        if hits.numel() < len(topk):
            raise ValueError("hits holds fewer counters than topk")
    if confusion is not None:
        check_input(confusion, "confusion", torch.int32)
        if confusion.numel() != C * C:
            raise ValueError(f"confusion must be ({C}, {C})")
    if bad_labels is not None:
        check_input(bad_labels, "bad_labels", torch.int32)
    if n == 0:      # (an empty tensor has no address to pass)
        return loss, lse
    alpha = None if weights is None else (ctypes.c_double * S)(*[float(w) for w in weights])
    ks = (ctypes.c_int * len(topk))(*topk) if topk else None
    with _timed("score_metrics", 0, scores.numel() * scores.element_size(), scores):
        rc = _lib.load().sgcn_score_metrics(
            _ptr(scores), n * C, S, alpha, int(scores.dtype == _F64), _ptr(labels), n, C,
            row_offset, _ptr(fused), _ptr(loss), _ptr(lse), _ptr(pred), _ptr(rank), ks,
            len(topk), _ptr(hits), _ptr(confusion), _ptr(bad_labels), _stream(scores))
    _lib.check(rc, "sgcn_score_metrics")
    return loss, lse


def batch_loss(loss, row_offset, n, out=None, batch_idx=0, mean_f32=None):
    """``sgcn_batch_loss``: mean of ``loss[row_offset : row_offset + n]`` into
    ``out[batch_idx]`` (float64) and / or ``mean_f32`` (a float32 scalar)."""
    check_input(loss, "loss", _F64)
    if loss.numel() < row_offset + n:
        raise ValueError("loss holds fewer rows than the batch")
    if out is not None:
        check_input(out, "batch_loss", _F64)
        if not 0 <= batch_idx < out.numel():
            raise ValueError("batch_idx outside batch_loss")
    if mean_f32 is not None:
        check_input(mean_f32, "mean_f32")
    if n == 0:
        return
    with _timed("batch_loss", 0, 8 * n, loss):
        rc = _lib.load().sgcn_batch_loss(_ptr(loss), row_offset, n, _ptr(out), batch_idx,
                                         _ptr(mean_f32), _stream(loss))
    _lib.check(rc, "sgcn_batch_loss")


def ce_bwd(logits, lse, labels, g):
    """``sgcn_ce_bwd``: the mean cross-entropy's gradient w.r.t. float32 ``logits`` (n, C);
    ``g`` is the loss's output gradient, a float32 device scalar."""
    check_input(logits, "logits")
    n, C = logits.shape
    check_input(lse, "lse", _F64)
    _check_labels(labels, n, logits.device)
    check_input(g, "grad_output")
    if lse.numel() < n or g.numel() != 1:
        raise ValueError("lse must hold n values and grad_output one")
    out = torch.empty_like(logits)
    if n == 0:
        return out
    with _timed("ce_bwd", 0, 8 * logits.numel(), logits):
        rc = _lib.load().sgcn_ce_bwd(_ptr(logits), _ptr(lse), _ptr(labels), _ptr(g), _ptr(out),
                                     n, C, _stream(logits))
    _lib.check(rc, "sgcn_ce_bwd")
    return out


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        logits = logits.contiguous()
        check_input(logits, "logits")
        if logits.dim() != 2 or logits.shape[0] == 0:
            raise ValueError("logits must be (n, C) with n >= 1")
        n = logits.shape[0]
        # {loss_i, lse_i} and the mean: device allocations only, two launches, no host read
        work = torch.empty((2, n), device=logits.device, dtype=_F64)
        mean = torch.empty((), device=logits.device, dtype=torch.float32)
        score_metrics(logits.detach(), labels, loss=work[0], lse=work[1])
        batch_loss(work[0], 0, n, mean_f32=mean)
        ctx.save_for_backward(logits, labels, work[1])
        return mean

    @staticmethod
    def backward(ctx, grad_output):
        logits, labels, lse = ctx.saved_tensors
        g = grad_output.to(torch.float32).contiguous()
        return ce_bwd(logits.detach(), lse, labels, g), None


def cross_entropy(logits, labels):
    """Mean cross-entropy of float32 ``logits`` (n, C) against int64 ``labels`` (n), as a
    float32 device scalar: ``mean_i(logsumexp(logits_i) - logits_i[label_i])`` evaluated in
    float64 in a fixed order (two launches forward, one backward; the same bits on every
    run). Safe under hipGraph capture: no host allocation, no synchronisation. A label outside
    ``[0, C)`` gives a NaN loss and a zero gradient row (there is no ``ignore_index``)."""
    return _CrossEntropy.apply(logits, labels)


class ScoreMetrics:
    """Device-side state of one evaluation run over ``num_class`` classes.

    ``topk``: up to 8 values of k. ``capacity``: rows of the run kept on the device (the
    fused score matrix, the predictions and the ranks of the label); without it only the
    counters and the per-batch losses are kept. ``update`` enqueues on the current stream and
    never synchronises; ``result`` makes the one device-to-host copy."""

    def __init__(self, num_class, topk=(1, 5), capacity=None, device="cuda"):
        self.num_class = int(num_class)
        self.topk = tuple(int(k) for k in topk)
        if self.num_class < 1:
            raise ValueError("num_class must be >= 1")
        if len(self.topk) > _lib.EVAL_MAX_K or any(k < 1 for k in self.topk):
            raise ValueError(f"topk: at most {_lib.EVAL_MAX_K} values, each >= 1")
        self.capacity = None if capacity is None else int(capacity)
        if self.capacity is not None and self.capacity < 1:
            raise ValueError("capacity must be >= 1 (or None: keep no rows)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ScoreMetrics runs on a CUDA device (there is no CPU path)")
        C = self.num_class
        # {hits[EVAL_MAX_K], bad_labels, confusion[C*C]}: zeroed by one fill
        self._counters = torch.zeros(_lib.EVAL_MAX_K + 1 + C * C, device=self.device,
                                     dtype=torch.int32)
        self._hits = self._counters[:_lib.EVAL_MAX_K]
        self._bad = self._counters[_lib.EVAL_MAX_K:_lib.EVAL_MAX_K + 1]
        self._confusion = self._counters[_lib.EVAL_MAX_K + 1:]
        # a batch has at least one row, so `capacity` batch slots always do
        self._batch_loss = torch.zeros(self.capacity or 256, device=self.device, dtype=_F64)
        self._scores = self._pred = self._rank = self._loss = None
        if self.capacity is not None:
            self._pred = torch.zeros(self.capacity, device=self.device, dtype=torch.int32)
            self._rank = torch.zeros(self.capacity, device=self.device, dtype=torch.int32)
            self._loss = torch.zeros((2, self.capacity), device=self.device, dtype=_F64)
        self.rows = 0       # host counters: nothing is read back to keep them
        self.batches = 0

    def reset(self):
        self._counters.zero_()
        self.rows = self.batches = 0

    def update(self, scores, labels, weights=None):
        """One batch: ``scores`` (n, C) float32 or float64, or (S, n, C) with S ``weights``
        (the fused row is then what the metrics are taken of, and what is kept)."""
        n, C = scores.shape[-2:]
        if C != self.num_class:
            raise ValueError(f"scores have {C} classes, the run {self.num_class}")
        if n == 0:
            return
        if self.batches == self._batch_loss.numel():   # (only without capacity) grow, on device
            grown = torch.zeros(2 * self.batches, device=self.device, dtype=_F64)
            grown[:self.batches].copy_(self._batch_loss)
            self._batch_loss = grown
        if self.capacity is not None:
            if self.rows + n > self.capacity:
                raise ValueError(f"run of {self.rows + n} rows exceeds capacity {self.capacity}")
            if self._scores is None:
                self._scores = torch.zeros((self.capacity, C), device=self.device,
                                           dtype=scores.dtype)
            elif self._scores.dtype != scores.dtype:
                raise RuntimeError("the run's scores changed dtype")
            off, loss, lse = self.rows, self._loss[0], self._loss[1]
        else:
            work = torch.empty((2, n), device=self.device, dtype=_F64)
            off, loss, lse = 0, work[0], work[1]
        score_metrics(scores, labels, weights, self.topk, off, self._scores, loss, lse,
                      self._pred, self._rank, self._hits, self._confusion, self._bad)
        batch_loss(loss, off, n, self._batch_loss, self.batches)
        self.rows += n
        self.batches += 1

    def result(self):
        """The run so far, as numpy / Python values (one device-to-host copy):
        ``mean_loss`` (mean of the batch means, float64: what main.py:508-509 prints),
        ``topk`` {k: accuracy}, ``confusion`` (C, C) [label, pred], ``per_class_accuracy``
        (NaN for a class without samples), ``batch_loss``, ``n``, and with ``capacity``
        ``pred``, ``rank``, ``scores`` (else None). Raises ValueError if any label was
        outside ``[0, num_class)``."""
        C, n, nb = self.num_class, self.rows, self.batches
        parts = {"batch_loss": self._batch_loss[:nb], "counters": self._counters}
        keep = self.capacity is not None and self._scores is not None
        if keep:
            parts.update(scores=self._scores[:n], pred=self._pred[:n], rank=self._rank[:n])
        # widest element type first, so every numpy view below is aligned
        order = sorted(parts, key=lambda name: -parts[name].element_size())
        flat = torch.cat([parts[name].reshape(-1).view(torch.uint8) for name in order])
        flat = flat.cpu().numpy()
        host, pos = {}, 0
        for name in order:
            t = parts[name]
            nbytes = t.numel() * t.element_size()
            dt = {torch.float64: np.float64, torch.float32: np.float32,
                  torch.int32: np.int32}[t.dtype]
            host[name] = flat[pos:pos + nbytes].view(dt).reshape(tuple(t.shape)).copy()
            pos += nbytes
        counters = host["counters"]
        bad = int(counters[_lib.EVAL_MAX_K])
        if bad:
            raise ValueError(f"{bad} labels outside [0, {C}) in the run")
        confusion = counters[_lib.EVAL_MAX_K + 1:].reshape(C, C).astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            per_class = np.diag(confusion) / confusion.sum(axis=1)
        return {
            "mean_loss": float(np.mean(host["batch_loss"])) if nb else float("nan"),
            "topk": {k: (int(counters[j]) / n if n else float("nan"))
                     for j, k in enumerate(self.topk)},
            "confusion": confusion,
            "per_class_accuracy": per_class,
            "batch_loss": host["batch_loss"],
            "n": n,
            "pred": host.get("pred"),
            "rank": host.get("rank"),
            "scores": host.get("scores"),
        }


def _host_labels(feeder, num_class):
    labels = np.asarray(feeder.label, dtype=np.int64)
    bad = np.flatnonzero((labels < 0) | (labels >= num_class))
    if bad.size:
        raise ValueError(f"{bad.size} labels outside [0, {num_class}) (first: sample "
                         f"{int(bad[0])}, label {int(labels[bad[0]])})")
    return labels


def evaluate_async(model, loader, topk=(1, 5)):
    """Enqueue the whole evaluation of ``model`` over ``loader`` and return the run's
    :class:`ScoreMetrics` without reading anything back (``.result()`` does). See
    :func:`evaluate`."""
    from .ensemble import Ensemble, EnsembleGraph
    if loader.shuffle:
        raise ValueError("evaluate needs a loader with shuffle=False (rows in dataset order)")
    if loader.world_size != 1:
        raise ValueError("evaluate runs on a single device (a sharded loader was given)")
    is_ens = isinstance(model, Ensemble)
    head = model.models[0] if is_ens else model
    if not is_ens and model.training:
        raise RuntimeError("evaluate runs the model in eval mode (call .eval())")
    num_class = head.fc.out_features
    _host_labels(loader.feeder, num_class)   # known on the host: checked once, up front
    rows = len(loader) * loader.batch_size if loader.drop_last else len(loader.feeder)
    metrics = ScoreMetrics(num_class, topk, capacity=max(rows, 1), device=loader.device)
    graph = None
    with torch.no_grad():
        for x, y, _ in loader:
            if not is_ens:
                scores = model(x)                       # float32 logits
            elif x.shape[0] == loader.batch_size:       # full batches: one hipGraph
                if graph is None:
                    graph = EnsembleGraph(model, tuple(x.shape), x.device)
                scores = graph.run(x)[1]                # float64 fused logits
            else:                                       # the short last batch, eagerly
                scores = model(x)[1]
            metrics.update(scores, y)
    return metrics


def evaluate(model, loader, topk=(1, 5), wrong_file=None, result_file=None, score_file=None):
    """``main.py:450-515`` for ``model`` (a :class:`Model` in ``.eval()``: float32 logits; or
    an :class:`Ensemble`: its float64 fused logits, full batches through one
    :class:`EnsembleGraph`) over ``loader`` (a :class:`DeviceBatchLoader` with
    ``shuffle=False``, single device). One forward and two small launches per batch, no
    host synchronisation inside the loop. Afterwards writes ``wrong_file``
    (``index,pred,true`` per wrong sample), ``result_file`` (``pred,true`` per sample) and
    ``score_file`` (the ``dict(zip(sample_name, score))`` pickle), and returns
    :meth:`ScoreMetrics.result`'s dict."""
    res = evaluate_async(model, loader, topk).result()
    n = res["n"]
    true = np.asarray(loader.feeder.label, dtype=np.int64)[:n]
    pred = res["pred"] if n else np.zeros(0, dtype=np.int32)
    if result_file is not None:
        with open(result_file, "w") as f:
            f.writelines(f"{int(p)},{int(t)}\n" for p, t in zip(pred, true))
    if wrong_file is not None:
        with open(wrong_file, "w") as f:
            f.writelines(f"{i},{int(p)},{int(t)}\n"
                         for i, (p, t) in enumerate(zip(pred, true)) if p != t)
    if score_file is not None:
        scores = res["scores"] if n else []
        with open(score_file, "wb") as f:
            pickle.dump(dict(zip(loader.feeder.sample_name, scores)), f)
    return res


def fuse_scores(score_dicts_or_arrays, labels, weights=(0.6, 0.6, 0.4, 0.4), topk=(1, 5),
                device="cuda"):
    """``ensemble.py`` for saved scores: each entry is a stream's ``sample_name -> score``
    dict (as ``main.py`` pickles it; rows in the dict's order, as the script reads them) or
    an (n, C) array. The float32 matrices are stacked into (S, n, C) and fused, scored and
    counted in ONE launch; ``labels`` is an (n,) integer sequence or the label pickle's
    ``(sample_name, label)`` pair. Returns :meth:`ScoreMetrics.result`'s dict; its
    ``scores`` are bit for bit ``r11*alpha[0] + r22*alpha[1] + ...`` on float32 arrays."""
    mats = []
    for s in score_dicts_or_arrays:
        if isinstance(s, dict):
            s = np.stack([np.asarray(v) for v in s.values()])
        mats.append(np.ascontiguousarray(s, dtype=np.float32))
    if len(mats) < 2 or len(mats) != len(weights):
        raise ValueError("fuse_scores takes two or more score streams and one weight each")
    if any(m.ndim != 2 or m.shape != mats[0].shape for m in mats):
        raise ValueError("every stream must hold the same (n, C) scores")
    if (isinstance(labels, (tuple, list)) and len(labels) == 2
            and not np.isscalar(labels[1]) and len(labels[0]) and isinstance(labels[0][0], str)):
        labels = labels[1]
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    n, C = mats[0].shape
    if labels.shape[0] != n:
        raise ValueError(f"{labels.shape[0]} labels for {n} score rows")
    stack = torch.from_numpy(np.stack(mats)).to(device)
    metrics = ScoreMetrics(C, topk, capacity=max(n, 1), device=device)
    metrics.update(stack, torch.from_numpy(labels).to(device), weights)
    return metrics.result()
