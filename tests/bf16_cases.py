"""Shape tables of the bf16-operand forward contraction's tests (sgcn_pw_fwd_bf16), the Python
mirror of its host chooser (``pw_fwd_bf16_form`` / ``kPwBf16Tiles``,
shift-gcn_amd/csrc/pw_forms.hpp) and the rounding the kernel applies to its operands (TEST
INFRASTRUCTURE ONLY). ``tests/test_bf16_forms.py`` holds the mirror equal to the C++ through
``tests/bf16_forms_dump.cpp``; ``tests/test_gpu_pw_bf16.py`` runs the tables."""
from __future__ import annotations

from oracle import pw_cases as pc
from oracle import pw_ref as pr  # noqa: F401  (the float64 restatement the GPU tests use)

K_BF16_BK = 32           # kPwBf16BK: k per LDS stage
K_MAX_K = pc.K_MAX_K     # kPwMaxK
BF16_TILES = [(64, 256, 2, 4), (128, 128, 4, 2), (256, 128, 4, 2)]   # kPwBf16Tiles


def bf16_form(M, K):
    """``pw_fwd_bf16_form``: the (bm, bn, wm, wn) tile; K does not enter."""
    return BF16_TILES[0 if M <= 64 else 1 if M <= 128 else 2]


def round_bf16(t):
    """Round to nearest even to bf16 and back (idempotent): what the kernel does to both
    operands on their way into LDS."""
    import torch
    return t.to(torch.bfloat16).to(t.dtype)


# M exact and ragged at every tile edge; two row blocks of the 256-row tile
BF16_MS = [1, 5, 64, 65, 128, 129, 300]
# K around the MFMA k-step (16), the stage (32) and the limit; every tile sees K mod 32 in
# {0, 1, 31} because the table is the full cross
BF16_KS = [1, 15, 16, 17, 31, 32, 33, 64, 65, 100, 255, 256]
FWD_PLANES = pc.FWD_PLANES
# one ragged (M, K) per tile for the flag crosses
BF16_FLAG_PAIRS = {(64, 256): (37, 100), (128, 128): (100, 65), (256, 128): (130, 33)}
BF16_FLAG_PLANES = [(3, 13, 25), (2, 9, 33)]
# one exact-integer case per tile (K at the limit: eight stages)
BF16_EXACT = {(64, 256): (64, 256), (128, 128): (100, 256), (256, 128): (300, 255)}


def flag_cases():
    """w_mcontig x relu x bias x y_rsign on the ragged pair of every tile."""
    out = []
    for tile, (M, K) in BF16_FLAG_PAIRS.items():
        i = 0
        for amc in (False, True):
            for relu in (False, True):
                for bias in (False, True):
                    for yr in (-1, 0, 1):
                        out.append(dict(M=M, K=K, plane=BF16_FLAG_PLANES[i % 2], w_mcontig=amc,
                                        relu=relu, bias=bias, y_rsign=yr))
                        i += 1
    return out
