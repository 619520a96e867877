"""Host side of the sequence pipeline: the two entry points reject bad arguments before
any launch (no GPU is touched), the new symbols are exported and bound, and a host window
table is checked before it is uploaded."""
import numpy as np
import pytest

from test_capi import declared_symbols

MP = (23, 11, 12, 11, 23, 24)        # z_bottom, z_top, x_right, x_left, center_a, center_b
P = 0x1000                           # a non-NULL pointer that is never dereferenced


def _normalize(lib, seq=P, table=P, out=P, n=2, T=100, V=33, M=1, W=48, joints=MP, stages=7):
    return lib.sgcn_window_normalize(seq, table, out, n, T, V, M, W, *joints, stages, None)


def test_symbols_exported_and_bound():
    from shiftgcn import _lib
    lib = _lib.load()
    for name in ("sgcn_window_normalize", "sgcn_window_aggregate"):
        assert name in declared_symbols() and name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["sgcn_window_normalize"][1]) == 16
    assert len(_lib.SIGNATURES["sgcn_window_aggregate"][1]) == 6
    assert _lib.ABI_VERSION == 25 == lib.sgcn_abi_version()
    from shiftgcn import pipeline
    for name in ("sliding_window_table", "normalize_windows", "aggregate_per_frame",
                 "detect_fall_intervals", "SequenceScorer", "MEDIAPIPE", "NTU"):
        assert hasattr(pipeline, name), name
    assert tuple(pipeline.MEDIAPIPE) == ((23, 11), (12, 11), (23, 24))
    assert tuple(pipeline.NTU) == ((0, 1), (8, 4), (1,))


def test_normalize_rejects_bad_arguments_before_launch():
    from shiftgcn import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    for kw in ({"seq": None}, {"table": None}, {"out": None}):
        assert _normalize(lib, **kw) == E, kw
    for pos in range(6):                                  # every joint index out of range
        for bad in (33, -2):
            j = list(MP)
            j[pos] = bad
            assert _normalize(lib, joints=j) == E, (pos, bad)
    assert _normalize(lib, V=24) == E                     # MediaPipe's joint 24 on 24 joints
    assert _normalize(lib, joints=(0, 1, 8, 4, 1, -1), V=25, M=2, seq=None) == E
    # the per-window frame maps must fit the LDS
    assert _normalize(lib, W=_lib.SEQ_MAX_WM + 1) == E
    assert _normalize(lib, W=_lib.SEQ_MAX_WM // 2 + 1, M=2) == E
    assert _normalize(lib, W=1 << 30, M=4) == E           # (no int overflow in W*M)
    for kw in ({"T": 0}, {"V": 0}, {"M": 0}, {"W": 0}, {"n": -1}, {"stages": 8},
               {"stages": -1}):
        assert _normalize(lib, **kw) == E, kw
    # an empty table is not an error and launches nothing (the pointers may be NULL)
    assert _normalize(lib, seq=None, table=None, out=None, n=0) == 0


def test_aggregate_rejects_bad_arguments_before_launch():
    from shiftgcn import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    assert lib.sgcn_window_aggregate(None, P, P, 3, 10, None) == E
    assert lib.sgcn_window_aggregate(P, None, P, 3, 10, None) == E
    assert lib.sgcn_window_aggregate(P, P, None, 3, 10, None) == E
    assert lib.sgcn_window_aggregate(P, P, P, -1, 10, None) == E
    assert lib.sgcn_window_aggregate(P, P, P, 3, -1, None) == E
    assert lib.sgcn_window_aggregate(None, None, None, 3, 0, None) == 0


def test_host_table_checked_before_upload():
    """The table lives on the device for the kernel, which can only clamp a bad row; a host
    table is refused here (the ValueError _lib.check raises for EINVAL)."""
    from shiftgcn import pipeline
    ok = pipeline.check_table([[0, 48], [24, 40]], 48, 64)
    assert ok.dtype == np.int32 and ok.flags.c_contiguous
    for bad, W, T in (([[0, 49]], 48, 100),               # num_real > W
                      ([[60, 48]], 48, 100),              # ends past the sequence
                      ([[-1, 4]], 48, 100), ([[0, -4]], 48, 100), ([0, 4], 48, 100)):
        with pytest.raises(ValueError):
            pipeline.check_table(bad, W, T)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        import torch
        pipeline.normalize_windows(torch.zeros(3, 8, 33, 1), ok, 48)
    for args in ((0, 300, 150), (10, 0, 1), (10, 4, 0)):
        with pytest.raises(ValueError):
            pipeline.sliding_window_table(*args)
    assert pipeline.sliding_window_table(10, 2, 20).tolist() == [[0, 2]]
    assert pipeline.sliding_window_table(10, 2, 3).tolist() == [[0, 2], [3, 2], [6, 2], [9, 1]]
