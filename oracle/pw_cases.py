"""Shape table of the contraction-kernel reference tests, and Python mirrors of the host
choosers that decide which kernel, tile and template instance a contraction runs (TEST
INFRASTRUCTURE ONLY).

``tests/test_gpu_pw_ref.py`` runs ``ops.pw_fwd`` / ``pw_dw`` / ``pw_fwd_tshift`` over the
tables below against ``oracle/pw_ref.py``; ``tests/test_oracle_pw.py`` checks, without a GPU,
that the tables reach every launch form a contraction CAN reach, by enumerating sizes
through the mirrors, and that the mirrors' split counts agree with the built library's
``sgcn_pw_dw_ws_bytes``. Each mirror restates one host function of
``shift-gcn_amd/csrc/pw_forms.hpp`` (the entry points of ``pwconv.hip`` call those and
nothing else decides a form); ``tests/test_launch_forms.py`` compiles that header into a host
program and holds the mirrors, the constants below and the header's tile lists equal to it
size by size. When a chooser changes, its mirror (and, if a new form appears, the table)
changes with it — the coverage test fails until the table reaches it.

Forms no size can reach (paths inside kernels that are launched, or forms that are not
built: every instantiated tile is reachable, ``tests/test_launch_forms.py``; kept — removing
them is not this table's business):

* ``pw_dw3_kernel`` 128 x 128 with a ragged tile: M <= 128, Nc <= 128 and M * Nc >= 16,384
  leave M = Nc = 128 only.
* ``pw_dw_kernel`` 128 x 128 on its plain fast path: a full 128 x 128 tile needs M >= 128
  and Nc >= 128, which is ``pw_dw3_kernel``'s; the PLAIN instance is launched (M, Nc in
  65..128 with M * Nc < 16,384) but always on its general loads.
* ``pw_dw_kernel`` with Nc <= 4, and every MFMA dW tile narrower than 5 columns:
  ``use_dwc`` takes them (``pw_dw_smallc_kernel``).
* ``pw_dw_smallc_kernel`` with an empty split below 256 positions per split (there S =
  ceil(P / 256) and every split holds a position).
* ``pw_fwd_smallm_kernel`` with a mask or a rotation (the chooser sends those to the MFMA
  tile), and the A-resident form on any tile but 64 x 256.
"""
from __future__ import annotations

# --------------------------------------------------------------------------------------
# mirrors of the host choosers (pw_forms.hpp)
# --------------------------------------------------------------------------------------
K_SMALL_M = 4            # kSmallM
K_DW_BK = 64             # kDwBK: pw_dw_kernel positions per chunk
K_DWC_ROWS = 16          # kDwcRows
K_DWC_MAX_C = 4          # kDwcMaxC
K_DW3_MIN = 128 * 128    # SGCN_DW3_MIN
K_DW3_BKP_BIG = 16       # SGCN_DW3_BKP_BIG
K_MASK_MAX_V = 64        # kMaskMaxV
K_MAX_K = 256            # kPwMaxK: sgcn_pw_fwd's K limit
K_EXTENT = 1 << 29       # kPwMaxElems: operand extents (elements) the buffer ranges accept


def _cdiv(a, b):
    return -(-a // b)


def fwd_form(M, K, mask=False, x_rsign=0, y_rsign=0, w_mcontig=False, accumulate=False):
    """``pw_fwd_form`` with ``sgcn_pw_fwd``'s flags: (family, tile, staging, flags). family
    "smallm" (``pw_fwd_smallm_kernel``, flags (AMC, ACCUM)) or "pwg" (``pwg_fwd_kernel``,
    staging "ar" = A-resident or "db" = double-buffered, flags (MASK, XROT, AMC, ACCUM))."""
    amc, acc = bool(w_mcontig), bool(accumulate)
    if M <= K_SMALL_M and not mask and x_rsign == 0 and y_rsign == 0:
        return ("smallm", None, None, (amc, acc))
    flags = (bool(mask), x_rsign != 0, amc, acc)
    if M <= 64:
        return ("pwg", (64, 256), "ar" if 16 < K <= 64 else "db", flags)
    if M <= 128:
        return ("pwg", (128, 128), "db", flags)
    return ("pwg", (256, 128), "db", flags)


def tshift_form(M):
    """``pw_tshift_form``: the tile of its ``pwg_fwd_kernel<TSH>``."""
    return (64, 256) if M <= 64 else (128, 256) if M <= 128 else (256, 128)


def use_dwc(Nc):
    """``use_dwc``."""
    return Nc <= K_DWC_MAX_C


def dwc_splits(M, P):
    """``dwc_splits``."""
    mg = _cdiv(M, 4 * K_DWC_ROWS)
    S = _cdiv(1024, mg)
    if _cdiv(P, S) < 256:
        S = _cdiv(P, 256)
    return max(S, 1)


def use_dw3(M, Nc):
    """``use_dw3``."""
    return M * Nc >= K_DW3_MIN


def dw3_cfg(M, Nc):
    """``dw3_cfg``: (bm, bn, bkp, target)."""
    if M <= 128 and Nc <= 128:
        return (128, 128, 16, 1024)
    if Nc <= 128:
        return (256, 128, K_DW3_BKP_BIG, 512)
    return (256, 256, K_DW3_BKP_BIG, 512)


def dw3_splits(M, Nc, P, bkp, tiles, target):
    """``dw3_splits``."""
    nch = _cdiv(P, bkp)
    S = min(_cdiv(target, tiles), (64 << 20) // (4 * M * Nc), nch)
    return max(S, 1)


def dw_tile(X):
    """``dw_tile``."""
    return 128 if X > 64 else 64


def dw_splits(M, Nc, B, N, tiles):
    """``dw_splits``."""
    total = B * _cdiv(N, K_DW_BK)
    S = min(_cdiv(512, tiles), (16 << 20) // (4 * M * Nc), total)
    return max(S, 1)


def dw_plain(mask, g_rsign, x_rsign, g_extent=0, x_extent=0):
    """``pw_dw_plain``."""
    return (not mask and g_rsign == 0 and x_rsign == 0 and g_extent < K_EXTENT and
            x_extent < K_EXTENT)


def dw_form(B, M, Nc, T, V, mask=False, g_rsign=0, x_rsign=0, dbias=False):
    """``pw_dw_form`` with ``sgcn_pw_dw``'s flags, and where its splits fall, a dict:

    family   "smallc" | "dw3" | "dw"
    tile     (bm, bn) (smallc: (NC,))
    flags    smallc (MASK,); dw3 (MASK, GROT, XROT, BIAS); dw "mask" | "plain" | "general"
    fast     dw: some workgroup takes the plain fast path (a full tile exists)
    S        split count (== the slab count of ``sgcn_pw_dw_ws_bytes``)
    per      chunks per split (smallc: positions per split); ``steps``: loop trips
    empty    trailing splits with no position
    mid      a non-empty split starts inside a sample (not at its first position)
    wraps    a split runs over a sample end (dw: the fast path's ``++fc == nchunk`` wrap)
    cross    dw3 / smallc: a chunk (64-position step) holds positions of two samples
    """
    N, P = T * V, B * T * V
    if use_dwc(Nc):
        S = dwc_splits(M, P)
        per = _cdiv(P, S)
        starts = [s * per for s in range(S) if s * per < P]
        ends = [min(q + per, P) for q in starts]
        return dict(family="smallc", tile=(Nc,), flags=(bool(mask),), fast=False, S=S, per=per,
                    steps=_cdiv(per, 64), empty=S - len(starts),
                    mid=any(q % N for q in starts),
                    wraps=any(q // N != (e - 1) // N for q, e in zip(starts, ends)),
                    cross=any(q // N != (min(q + 64, e) - 1) // N
                              for q0, e in zip(starts, ends) for q in range(q0, e, 64)))
    if use_dw3(M, Nc):
        bm, bn, bkp, target = dw3_cfg(M, Nc)
        tiles = _cdiv(M, bm) * _cdiv(Nc, bn)
        S = dw3_splits(M, Nc, P, bkp, tiles, target)
        nch = _cdiv(P, bkp)
        cps = _cdiv(nch, S)
        starts = [s * cps for s in range(S) if s * cps < nch]
        ends = [min(q + cps, nch) for q in starts]
        return dict(family="dw3", tile=(bm, bn),
                    flags=(bool(mask), g_rsign != 0, x_rsign != 0, bool(dbias)), fast=False,
                    S=S, per=cps, steps=cps, empty=S - len(starts),
                    mid=any((q * bkp) % N for q in starts),
                    wraps=any((q * bkp) // N != (min(e * bkp, P) - 1) // N
                              for q, e in zip(starts, ends)),
                    cross=any((q * bkp) // N != (min((q + 1) * bkp, P) - 1) // N
                              for q in range(nch)),
                    ragged_last=P % bkp != 0)
    bm, bn = dw_tile(M), dw_tile(Nc)
    tiles = _cdiv(M, bm) * _cdiv(Nc, bn)
    S = dw_splits(M, Nc, B, N, tiles)
    nchunk = _cdiv(N, K_DW_BK)
    total = B * nchunk
    cps = _cdiv(total, S)
    starts = [s * cps for s in range(S) if s * cps < total]
    ends = [min(q + cps, total) for q in starts]
    plain = dw_plain(mask, g_rsign, x_rsign)
    return dict(family="dw", tile=(bm, bn),
                flags="mask" if mask else "plain" if plain else "general",
                fast=plain and M >= bm and Nc >= bn, S=S, per=cps, steps=cps,
                empty=S - len(starts), mid=any(q % nchunk for q in starts),
                wraps=any(q // nchunk != (e - 1) // nchunk for q, e in zip(starts, ends)),
                cross=False)


def dw_ws_bytes(B, M, Nc, T, V):
    """``sgcn_pw_dw_ws_bytes`` from the mirror's split count."""
    return dw_form(B, M, Nc, T, V)["S"] * (M * Nc + M) * 4


# --------------------------------------------------------------------------------------
# weight gradient: (B, M, Nc, T, V)
# --------------------------------------------------------------------------------------
DW_TABLE = [
    (8, 64, 64, 192, 25),     # dw 64 x 64: S = 512, 2 chunks per split, 212 empty splits
    (11, 128, 64, 120, 25),   # dw 128 x 64 on the fast path: 2 chunks per split, 47 per sample
    (11, 64, 128, 120, 25),   # dw 64 x 128 likewise
    (11, 64, 64, 91, 33),     # the same wrap at V = 33
    (6, 100, 64, 150, 33),    # dw 128 x 64, ragged M
    (6, 64, 100, 150, 33),    # dw 64 x 128, ragged Nc
    (4, 100, 100, 146, 33),   # dw 128 x 128
    (3, 64, 64, 64, 64),      # V = 64: dt = 1, dv = 0; the mask's V limit
    (2, 40, 37, 9, 70),       # V > 64 (no mask)
    (9, 48, 40, 1, 1),        # V = 1, T * V far below one chunk
    (3, 129, 128, 171, 33),   # dw3 256 x 128: 3 chunks per split, 159 empty, ragged last chunk
    (2, 64, 256, 321, 25),    # dw3 256 x 256
    (3, 200, 130, 213, 33),   # dw3 256 x 256, both ragged
    (3, 128, 128, 320, 25),   # dw3 128 x 128: 2 chunks per split, 274 empty splits
    (8, 100, 3, 656, 25),     # smallc: 257 positions per split, one empty split
    (2, 17, 1, 5, 25),        # smallc Nc = 1, one ragged wave of rows
    (3, 100, 2, 7, 33),       # smallc Nc = 2, M no multiple of 16 or 64, two splits
    (2, 70, 4, 3, 25),        # smallc Nc = 4, two row groups
    (4, 64, 3, 17, 25),       # smallc Nc = 3: l1's gcn Linear
    # the small shapes the flag crosses run on (two per tile)
    (3, 64, 64, 5, 25), (2, 37, 51, 9, 33),          # dw 64 x 64
    (2, 128, 64, 7, 25), (3, 100, 40, 5, 33),        # dw 128 x 64 (full first: fast path)
    (2, 64, 128, 7, 25), (3, 40, 100, 5, 33),        # dw 64 x 128
    (2, 100, 100, 5, 25), (3, 70, 128, 3, 33),       # dw 128 x 128
    (2, 128, 128, 5, 25), (3, 128, 128, 3, 33),      # dw3 128 x 128
    (2, 129, 128, 5, 25), (3, 300, 60, 3, 33),       # dw3 256 x 128 (two M tiles)
    (2, 129, 129, 5, 25), (3, 64, 257, 3, 33),       # dw3 256 x 256 (two Nc tiles)
]

# per (family, tile): the two shapes every flag combination runs on
DW_FLAG_SHAPES = {
    ("dw", (64, 64)): [(3, 64, 64, 5, 25), (2, 37, 51, 9, 33)],
    ("dw", (128, 64)): [(2, 128, 64, 7, 25), (3, 100, 40, 5, 33)],
    ("dw", (64, 128)): [(2, 64, 128, 7, 25), (3, 40, 100, 5, 33)],
    ("dw", (128, 128)): [(2, 100, 100, 5, 25), (3, 70, 128, 3, 33)],
    ("dw3", (128, 128)): [(2, 128, 128, 5, 25), (3, 128, 128, 3, 33)],
    ("dw3", (256, 128)): [(2, 129, 128, 5, 25), (3, 300, 60, 3, 33)],
    ("dw3", (256, 256)): [(2, 129, 129, 5, 25), (3, 64, 257, 3, 33)],
    ("smallc", (3,)): [(4, 64, 3, 17, 25), (3, 100, 2, 7, 33)],
}

# operand forms every DW_TABLE shape runs in: (g_rsign, x_rsign, mask)
DW_OPERANDS = [(0, 0, False), (1, -1, False), (-1, 1, True)]
RSIGNS = (0, 1, -1)

# cases at or below this many positions keep the fixed bar; larger ones measure theirs
DW_FIXED_BAR_POSITIONS = 1700


# --------------------------------------------------------------------------------------
# forward / dX: (M, K) pairs and (B, T, V) planes
# --------------------------------------------------------------------------------------
FWD_PAIRS = [
    (1, 1), (1, 3), (4, 64), (4, 256),       # smallm: up to its M limit, K at both ends
    (5, 16), (5, 17), (64, 64), (64, 65),    # 64 x 256: 4|5, K 16|17 (db|ar), 64|65 (ar|db)
    (37, 100), (64, 1), (33, 3),             # ... double-buffered, ragged M and K
    (17, 51), (64, 17),                      # ... A-resident, ragged M and K
    (65, 64), (65, 3), (128, 65), (100, 256), (128, 16),   # 128 x 128: 64|65 up to 128
    (129, 17), (129, 100), (300, 16), (300, 256), (256, 1),   # 256 x 128: 128|129, 2 M-blocks
]
FWD_PLANES = [
    (1, 2, 25),     # P = 50: less than one position tile
    (2, 128, 1),    # P = 256: an exact tile; V = 1
    (3, 13, 25),    # several tiles, ragged last, tiles spanning samples
    (2, 9, 33),
    (1, 3, 70),     # V > 64: no mask
    (2, 5, 64),     # V = 64: the mask's limit
]
# one ragged (M, K) per (tile, staging) for the flag crosses, on plane (3, 13, 25) / (2, 9, 33)
FWD_FLAG_PAIRS = {
    ((64, 256), "ar"): (37, 51),
    ((64, 256), "db"): (37, 100),
    ((128, 128), "db"): (100, 37),
    ((256, 128), "db"): (130, 37),
}
FWD_FLAG_PLANES = [(3, 13, 25), (2, 9, 33)]
SMALLM_PAIRS = [(3, 64), (4, 130)]

# fused temporal shift: (B, K, M, T, V), the order of tests/test_gpu_tshift_fused.py
TSHIFT_CASES = [
    (3, 64, 64, 20, 25),
    (2, 128, 128, 17, 25),
    (2, 256, 256, 9, 25),
    (2, 100, 37, 9, 25),     # ragged K: rows clamped to K - 1; 64 x 256 tile
    (2, 37, 130, 7, 33),     # ragged K and M on the 256 x 128 tile
    (1, 40, 300, 5, 25),     # M > 256: two M-blocks form (and store) the side output
    (2, 40, 100, 5, 25),     # the 128 x 256 tile, ragged
]


def fwd_flag_cases():
    """Every (tile, staging, MASK, XROT, AMC, ACCUM) instance of ``pwg_fwd_kernel`` and the
    four of ``pw_fwd_smallm_kernel``: dicts of pw_fwd arguments."""
    out = []
    for (tile, stage), (M, K) in FWD_FLAG_PAIRS.items():
        for i, (mask, xrot, amc, acc) in enumerate(
                (a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)):
            out.append(dict(M=M, K=K, plane=FWD_FLAG_PLANES[i % 2], mask=bool(mask),
                            x_rsign=(1 if i % 4 < 2 else -1) if xrot else 0,
                            y_rsign=(0, 1, -1)[i % 3], w_mcontig=bool(amc),
                            accumulate=bool(acc), relu=bool(i & 1), bias=i % 5 != 0))
    for M, K in SMALLM_PAIRS:
        for amc in (0, 1):
            for acc in (0, 1):
                out.append(dict(M=M, K=K, plane=FWD_FLAG_PLANES[amc], mask=False, x_rsign=0,
                                y_rsign=0, w_mcontig=bool(amc), accumulate=bool(acc),
                                relu=bool(acc), bias=bool(amc)))
    return out


def fwd_rsign_cases():
    """x_rsign, y_rsign in {-1, 0, +1} on every MFMA (tile, staging), masked or not."""
    out = []
    for (M, K) in FWD_FLAG_PAIRS.values():
        for xr in RSIGNS:
            for yr in RSIGNS:
                out.append(dict(M=M, K=K, plane=FWD_FLAG_PLANES[(xr + yr) % 2],
                                mask=(xr * yr) != 0, x_rsign=xr, y_rsign=yr, w_mcontig=xr > 0,
                                accumulate=False, relu=yr > 0, bias=True))
    return out


def fwd_case_form(c):
    return fwd_form(c["M"], c["K"], c["mask"], c["x_rsign"], c["y_rsign"], c["w_mcontig"],
                    c["accumulate"])


# --------------------------------------------------------------------------------------
# deterministic inputs: float32 on the CPU, unit variance (weights randn / sqrt(K))
# --------------------------------------------------------------------------------------
def rnd(shape, seed, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(*shape, generator=g) * scale


def mask_values(V, C, seed):
    """tanh(Feature_Mask) + 1 lies in (0, 2): uniform in [0.5, 1.5)."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return torch.rand(V, C, generator=g) + 0.5
