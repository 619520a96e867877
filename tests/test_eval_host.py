"""Evaluation on the device, the parts that need no GPU: the new C-ABI symbols and their
argument checks, and the rank rule itself.

The rank rule of ``sgcn_score_metrics`` (include/shiftgcn.h), stated here in numpy
(:func:`rank_rule`; tests/test_gpu_eval.py holds the kernel to it exactly):

    rank_i = #{c : r[c] > r[l]} + #{c > l : r[c] == r[l]},   hit at k  iff  rank_i < k

which is ``l in np.argsort(r, kind="stable")[-k:]``. ``Feeder.top_k`` sorts with numpy's
default kind, which is not stable, so it is compared on tie-free scores only.
"""
import ctypes
import pickle

import numpy as np
import pytest

NEW_SYMBOLS = ("sgcn_score_metrics", "sgcn_batch_loss", "sgcn_ce_bwd")


def rank_rule(scores, labels):
    """(n,) rank of each row's label; C for a label outside [0, C)."""
    scores = np.asarray(scores)
    n, C = scores.shape
    out = np.full(n, C, dtype=np.int64)
    for i, l in enumerate(labels):
        if 0 <= l < C:
            r = scores[i]
            out[i] = int((r > r[l]).sum() + (r[l + 1:] == r[l]).sum())
    return out


def pred_rule(scores):
    """First index of the maximum (np.argmax)."""
    return np.argmax(np.asarray(scores), axis=1)


def stable_hits(scores, labels, k):
    order = np.argsort(scores, axis=1, kind="stable")
    return np.array([l in order[i, -k:] for i, l in enumerate(labels)])


def test_library_exports_the_evaluation_symbols():
    from shiftgcn import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == list(args)
    assert len(_lib.SIGNATURES["sgcn_score_metrics"][1]) == 20
    assert len(_lib.SIGNATURES["sgcn_batch_loss"][1]) == 7
    assert len(_lib.SIGNATURES["sgcn_ce_bwd"][1]) == 8


def test_abi_version_is_still_25():
    from shiftgcn import _lib
    assert _lib.load().sgcn_abi_version() == 25 == _lib.ABI_VERSION


def _metrics_call(lib, **over):
    """sgcn_score_metrics with host memory standing in for every pointer: only ever used with
    arguments that must be refused (or n = 0), so nothing is launched or dereferenced."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(scores=p, stride=0, S=1, alpha=None, f64=0, labels=p, n=4, C=5, off=0, fused=None,
             loss=p, lse=p, pred=None, rank=None, k=None, nk=0, hits=None, confusion=None,
             bad=None)
    a.update(over)
    return lib.sgcn_score_metrics(a["scores"], a["stride"], a["S"], a["alpha"], a["f64"],
                                  a["labels"], a["n"], a["C"], a["off"], a["fused"], a["loss"],
                                  a["lse"], a["pred"], a["rank"], a["k"], a["nk"], a["hits"],
                                  a["confusion"], a["bad"], None), buf


def test_invalid_arguments_rejected_before_launch():
    from shiftgcn import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    for name in ("scores", "labels", "loss", "lse"):          # NULL required pointers
        assert _metrics_call(lib, **{name: None})[0] == E, name
    for C in (0, -3):
        assert _metrics_call(lib, C=C)[0] == E
    alpha = (ctypes.c_double * 9)(*([0.5] * 9))
    for S in (0, -1, 9):
        assert _metrics_call(lib, S=S, alpha=alpha, stride=20)[0] == E
    assert _metrics_call(lib, S=2, alpha=None, stride=20)[0] == E   # weights missing
    ks = (ctypes.c_int * 9)(*range(1, 10))
    buf = ctypes.create_string_buffer(64)
    assert _metrics_call(lib, k=ks, nk=9, hits=ctypes.addressof(buf))[0] == E
    assert _metrics_call(lib, k=ks, nk=2, hits=None)[0] == E
    assert _metrics_call(lib, n=-1)[0] == E
    assert _metrics_call(lib, off=-1)[0] == E
    # n == 0: success, nothing launched
    assert _metrics_call(lib, n=0)[0] == 0
    p = ctypes.addressof(buf)
    assert lib.sgcn_batch_loss(None, 0, 4, p, 0, None, None) == E
    assert lib.sgcn_batch_loss(p, 0, 4, None, 0, None, None) == E
    assert lib.sgcn_batch_loss(p, 0, -1, p, 0, None, None) == E
    assert lib.sgcn_batch_loss(p, 0, 0, p, 0, None, None) == 0
    assert lib.sgcn_ce_bwd(None, p, p, p, p, 4, 5, None) == E
    assert lib.sgcn_ce_bwd(p, p, p, None, p, 4, 5, None) == E
    assert lib.sgcn_ce_bwd(p, p, p, p, None, 4, 5, None) == E
    assert lib.sgcn_ce_bwd(p, p, p, p, p, 4, 0, None) == E
    assert lib.sgcn_ce_bwd(p, p, p, p, p, 0, 5, None) == 0
    assert buf.raw == b"\0" * 64


def _feeder(tmp_path, labels):
    from shiftgcn.feeder import Feeder
    n = len(labels)
    np.save(tmp_path / "d.npy", np.zeros((n, 1, 1, 1, 1), dtype=np.float32))
    with open(tmp_path / "l.pkl", "wb") as f:
        pickle.dump(([f"s{i}" for i in range(n)], [int(v) for v in labels]), f)
    return Feeder(str(tmp_path / "d.npy"), str(tmp_path / "l.pkl"))


@pytest.mark.parametrize("C", [2, 5, 60])
def test_rank_rule_equals_feeder_top_k_on_tie_free_scores(tmp_path, C):
    rng = np.random.default_rng(C)
    n = 200
    scores = rng.permuted(np.tile(np.arange(C, dtype=np.float32), (n, 1)), axis=1)
    scores = scores * np.float32(0.37) - np.float32(3)          # distinct within a row
    labels = rng.integers(0, C, n)
    fd = _feeder(tmp_path, labels)
    rank = rank_rule(scores, labels)
    for k in (1, 5):
        assert (rank < k).mean() == fd.top_k(scores, k)
        assert np.array_equal(rank < k, stable_hits(scores, labels, k))
    assert np.array_equal(rank == 0, pred_rule(scores) == labels)


@pytest.mark.parametrize("C", [2, 5, 60, 65])
def test_rank_rule_equals_stable_argsort_with_ties(C):
    rng = np.random.default_rng(100 + C)
    n = 300
    scores = rng.integers(0, 3, (n, C)).astype(np.float32)      # 3 distinct values
    labels = rng.integers(0, C, n)
    # the label at both ends of a tie group: the first and the last index of its value
    for i in range(0, n, 3):
        same = np.flatnonzero(scores[i] == scores[i, labels[i]])
        labels[i] = same[0] if i % 2 else same[-1]
    rank = rank_rule(scores, labels)
    for k in (1, 2, 5, C, C + 3):
        assert np.array_equal(rank < k, stable_hits(scores, labels, min(k, C))), k
    # position from the top of the stable ascending order
    order = np.argsort(scores, axis=1, kind="stable")
    pos = np.array([C - 1 - int(np.flatnonzero(order[i] == l)[0]) for i, l in enumerate(labels)])
    assert np.array_equal(rank, pos)
    assert np.array_equal(rank_rule(scores[:2], [-1, C]), [C, C])


def test_public_surface():
    import shiftgcn
    from shiftgcn import train
    from shiftgcn.evaluate import ScoreMetrics, evaluate_async
    for name in ("ScoreMetrics", "evaluate", "fuse_scores"):
        assert name in shiftgcn.__all__ and callable(getattr(shiftgcn, name))
    assert callable(train.cross_entropy) and callable(evaluate_async)
    import inspect
    assert inspect.signature(train.train_step).parameters["loss_fn"].default is None
    with pytest.raises(ValueError):
        ScoreMetrics(5, topk=tuple(range(1, 10)), device="cuda")
