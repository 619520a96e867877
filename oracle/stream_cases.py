"""Shape table of the streaming-kernel reference tests, and Python mirrors of the launch
choosers that decide which kernel instantiation a (T, V) plane runs (TEST INFRASTRUCTURE
ONLY).

``tests/test_gpu_stream_ref.py`` runs every op over :data:`TABLE` (+ :data:`SHIFT_EXTRA` for
the shift-fused ops); ``tests/test_oracle_stream.py`` checks, without a GPU, that those
shapes reach every launch form a plane CAN reach, by enumerating all planes through the
mirrors below. Each mirror restates one host function of
``shift-gcn_amd/csrc/launch_forms.hpp`` (the entry points call those, so they are the
library's decision); ``tests/test_launch_forms.py`` compiles that header into a host program
and compares it with the mirrors on every plane. When a chooser changes, its mirror (and, if
a new form appears, the table) changes with it — the coverage test fails until the table
reaches the new form.

Forms no plane can reach. They are no longer built: a launcher instantiates its form list in
``launch_forms.hpp``, which the same test holds equal to the forms the chooser returns (a
form outside the list is refused with SGCN_EINVAL, never mapped to another):

* BatchNorm plane kernels and ``gcn_dx_finish_ja_kernel``: 512 x 8 and 512 x 16. 512
  threads are chosen only above 8,192 floats, and (512 / V) * V <= 512 lanes then hold at
  least 17 elements each.
* padded forward (``tshift_fwd_pad_kernel`` behind ``sgcn_tshift_fwd_pre`` / ``_tail``):
  512 x 8, 512 x 12 and 512 x 16, for the same reason (512 threads above 8,192 floats);
  behind ``sgcn_tshift_fwd`` also 256 x 12 and 256 x 20 (12 and 20 are 512-thread counts).
* stride-1 backward behind ``sgcn_tshift_bwd_bnin``: 512 x 8 (512 threads above 4,096
  floats: at least 9 per lane) and 256 x 32 (256 threads up to 4,096 floats; the
  narrowest joint-aligned stride of any V <= 64 is 208 lanes (V = 52): at most 20 per
  lane).
"""
from __future__ import annotations

# --------------------------------------------------------------------------------------
# mirrors of the launch choosers
# --------------------------------------------------------------------------------------
K_JA_SPLIT = 8192        # launch_forms.hpp kJaSplit
K_FWD_LDS_MAX = 8192     # launch_forms.hpp kFwdLdsMax
K_FWD_LDS_MAX2 = 16384   # launch_forms.hpp kFwdLdsMax2
K_BWD_LDS_MAX = 16384    # launch_forms.hpp kBwdLdsMax
K_PAD_ROWS = 4           # launch_forms.hpp kPadRows
K_BNIN_SPLIT = 4096      # launch_forms.hpp kBninSplit
K_LDS_BYTES = 65536      # launch_forms.hpp kRaLdsMax / pad_fwd_lpt's 64 KiB
K_PLANE_V_MAX = 256      # bn.hip SGCN_PLANE_CHECK: V <= kThreads


def _bucket(per):
    return 8 if per <= 8 else 16 if per <= 16 else 24 if per <= 24 else 32 if per <= 32 else 0


def ja_lpt(T, V, nt):
    """launch_forms.hpp ``ja_lpt``."""
    if V > 64:
        return 0
    ntj = (nt // V) * V
    return _bucket(-(-T * V // ntj))


def bn_form(T, V):
    """Launch form of sgcn_moments / sgcn_bn_apply / sgcn_bn_bwd_reduce / sgcn_bn_bwd_apply /
    sgcn_gcn_dx_finish (launch_forms.hpp ``bn_form``):
    ("ja", threads, per-thread), "loop" (the looping kernels) or "refuse" (SGCN_PLANE_CHECK)."""
    if V > K_PLANE_V_MAX:
        return "refuse"
    nt = 256 if T * V <= K_JA_SPLIT else 512
    lpt = ja_lpt(T, V, nt)
    return ("ja", nt, lpt) if lpt else "loop"


def ra_pad_floats(H, W):
    """launch_forms.hpp ``ra_pad_floats``."""
    return (H + 2 * K_PAD_ROWS) * (W + 2)


def pad_lds_fits(H, W):
    """The pad-LDS limit of launch_forms.hpp ``pad_fwd_lpt`` / ``ra_lds_bytes`` (without
    GBN): the padded plane + one spare float within 64 KiB."""
    return (ra_pad_floats(H, W) + 1) * 4 <= K_LDS_BYTES


def pad_fwd_lpt(H, W, nt):
    """launch_forms.hpp ``pad_fwd_lpt``."""
    if W > 64:
        return 0
    ntj = (nt // W) * W
    per = -(-H * W // ntj)
    lpt = _bucket(per)
    if nt == 512 and 8 < per <= 12:
        lpt = 12
    if nt == 512 and 16 < per <= 20:
        lpt = 20
    return lpt if pad_lds_fits(H, W) else 0


def pick_lpt(n, nt):
    """launch_forms.hpp ``pick_lpt``."""
    per = -(-n // nt)
    return 8 if per <= 8 else 16 if per <= 16 else 32


def fwd_form(H, W):
    """Launch form of sgcn_tshift_fwd_pre / sgcn_tshift_fwd_tail (launch_forms.hpp
    ``fwd_fused_form``, where "fallback" is the kind ``lds``): ("pad", threads, per-thread), ("fallback", threads, per-thread)
    (tshift_fwd_pre_kernel / tshift_fwd_tail_kernel) or "refuse" (H * W > kFwdLdsMax2)."""
    n = H * W
    if n > K_FWD_LDS_MAX2 or W > 1024:
        return "refuse"
    nt = 256 if n <= K_FWD_LDS_MAX else 512
    lpt = pad_fwd_lpt(H, W, nt)
    if lpt:
        return ("pad", nt, lpt)
    if n <= K_FWD_LDS_MAX:
        return ("fallback", 256, pick_lpt(n, 256))
    return ("fallback", 512, 32)


def ra_lpt(n, nt, W):
    """launch_forms.hpp ``ra_lpt``."""
    nte = (nt // W) * W
    if nte <= 0 or W > 64:
        return 0
    per = -(-n // nte)
    if nt == 512 and 8 < per <= 12:
        return 12
    if nt == 512 and 16 < per <= 20:
        return 20
    return _bucket(per)


def bnin_form(H, W):
    """Launch form of sgcn_tshift_bwd_bnin (launch_forms.hpp ``bnin_form``):
    ("ra", threads, per-thread) or "refuse" (SGCN_EINVAL; ``ops.ra_fits`` is False)."""
    n = H * W
    if n > K_BWD_LDS_MAX:
        return "refuse"
    nt = 256 if n <= K_BNIN_SPLIT else 512
    lpt = ra_lpt(n, nt, W)
    if lpt == 0 or not pad_lds_fits(H, W):
        return "refuse"
    return ("ra", nt, lpt)


def reachable(form, v_max=K_PLANE_V_MAX, n_max=K_FWD_LDS_MAX2 + 2 * K_PLANE_V_MAX):
    """Every value ``form(T, V)`` takes over the planes a launcher accepts (V <= v_max,
    T * V <= n_max: past the largest threshold nothing new can appear), "refuse" excluded."""
    out = set()
    for V in range(1, v_max + 1):
        for T in range(1, n_max // V + 2):
            f = form(T, V)
            if f != "refuse":
                out.add(f)
    return out


# --------------------------------------------------------------------------------------
# the shape table: (B, C, T, V)
# --------------------------------------------------------------------------------------
TABLE = [
    (2, 5, 7, 25),       # 256 x 8, ragged plane, C % V != 0
    (1, 53, 3, 25),      # c >= V: the rotation wraps twice
    (1, 2, 1, 25),       # T = 1
    (1, 2, 5, 1),        # V = 1
    (1, 3, 80, 25),      # 2,000 = 250 x 8 exactly full
    (1, 3, 81, 25),      # one row more: 256 x 16
    (1, 3, 161, 25),     # 256 x 24
    (2, 3, 300, 25),     # 256 x 32, the NTU plane
    (1, 2, 320, 25),     # 8,000 = 250 x 32 exactly full
    (1, 2, 325, 25),     # <= 8,192 floats but 33 per thread: looping kernels at V <= 64
    (1, 2, 328, 25),     # first 512-thread plane, 512 x 24
    (1, 3, 300, 33),     # MediaPipe: 9,900 = 495 x 20 exactly (shift 512 x 20, BatchNorm 512 x 24)
    (1, 2, 301, 33),     # one row over
    (1, 2, 240, 33),     # 7,920 floats: BatchNorm loops, the shift backward takes 512 threads
    (1, 2, 128, 64),     # V = 64: no idle threads, 8,192 = 256 x 32 exactly
    (1, 2, 129, 64),     # then 512 x 24
    (1, 2, 640, 25),     # 16,000 = 500 x 32 exactly
    (1, 2, 641, 25),     # then looping; bnin refuses
    (1, 2, 9, 70),       # V > 64: looping
    (1, 2, 3, 256),      # V = 256 = workgroup width (G = 1)
]

# further shapes of the shift-fused ops (tshift_fwd_pre / _tail / tshift_bwd_bnin)
SHIFT_EXTRA = [
    (1, 2, 163, 25),     # bnin 256 x 24: the last plane of <= 4,096 floats at V = 25
    (1, 2, 164, 25),     # bnin 512 x 12
    (1, 2, 598, 25),     # the padded plane just fits 64 KiB
    (1, 2, 599, 25),     # it does not: pre / tail fall back to 512 x 32, bnin refuses
    (1, 2, 40, 70),      # W > 64: fallback 256 x 16
    (1, 2, 60, 70),      # fallback 256 x 32 (W > 64, 4,097..8,192 floats)
]
SHIFT_TABLE = TABLE + SHIFT_EXTRA

# stride-2 cases of tshift_fwd_pre / _tail: odd H (the last input row feeds no output)
STRIDE2 = [(1, 2, 21, 25), (1, 3, 81, 25), (1, 2, 301, 25), (1, 2, 301, 33)]

# shapes the argument forms that share one instantiation set are run on: one 256-thread
# plane (the ragged first case), one 512-thread plane, one looping plane
FORM_SHAPES = [(2, 5, 7, 25), (1, 3, 300, 33), (1, 2, 9, 70)]


def shift_positions(C, H, variant):
    """(xpos, ypos) lists of C float values for one shift case. Channel c takes entry
    (c + C * variant) of an 8-entry cycle, so ``n_variants(C)`` variants put every entry on
    some channel: xpos ~ +-1e-8 and one each of 1.5, -2.25 and 0; ypos in +-3.5 with 0 and
    an integer; one |ypos| > 4 (past the padding: the range-checked loop); one |ypos| > H
    (every tap out of range)."""
    cycle = [
        (0.9e-8, 0.0),
        (-0.7e-8, 2.0),
        (1.5, -3.5),
        (-2.25, 1.3),
        (0.0, 3.5),
        (0.4e-8, 5.5),
        (-0.3e-8, -(H + 1.5)),
        (0.6e-8, -0.75),
    ]
    pick = [cycle[(c + C * variant) % 8] for c in range(C)]
    return [p[0] for p in pick], [p[1] for p in pick]


def n_variants(C):
    return -(-8 // C)


# --------------------------------------------------------------------------------------
# deterministic inputs (tests/golden/formula.py seeds), float32 on the CPU
# --------------------------------------------------------------------------------------
def t(shape, seed, scale=1.0, offset=0.0):
    import formula
    return formula.tensor(tuple(shape), seed, scale, offset)


def act(shape, seed):
    """A tensor that feeds a ``> 0`` predicate: positives, negatives, exact +0.0 and -0.0
    (every second zero), the first four elements one of each whatever the seed gives."""
    import torch
    v = t(shape, seed)
    flat = torch.where(v.abs() < 0.2, torch.zeros_like(v), v).reshape(-1)
    flat[:4] = torch.tensor([0.0, -0.0, 0.5, -0.5])[:flat.numel()]
    z = (flat == 0).nonzero().reshape(-1)
    flat[z[1::2]] = -0.0
    return flat.reshape(shape)


def has_all_signs(v):
    """positives, negatives, +0.0 and -0.0 all present."""
    import torch
    z = v == 0
    return bool((v > 0).any() and (v < 0).any() and (z & ~torch.signbit(v)).any() and
                (z & torch.signbit(v)).any())


def positions(C, H, variant):
    import torch
    xp, yp = shift_positions(C, H, variant)
    return torch.tensor(xp, dtype=torch.float32), torch.tensor(yp, dtype=torch.float32)


def bnin_inputs(shape, variant, plane_dy=False):
    """(dy, y, s, coef, inp, xpos, ypos) of one sgcn_tshift_bwd_bnin case."""
    B, C, H, W = shape
    sd = 100 * variant
    dy = t((B, C), 50 + sd) if plane_dy else t(shape, 51 + sd)
    y, s, inp = act(shape, 52 + sd), t(shape, 53 + sd), act(shape, 54 + sd)
    coef = t((3, C), 55 + sd, 0.5, 0.25)
    xpos, ypos = positions(C, H, variant)
    return dy, y, s, coef, inp, xpos, ypos


GY_REL = 1e-4   # a channel's fp64 batch-mean position sum counts as sign-robust above
                # GY_REL x mean |per-plane sum| (DESIGN row a6)


def gy_unsafe(part, mean):
    """Channels whose finalized gy is not robust: 0 < |fp64 batch mean| <= GY_REL x mean
    |per-plane y sum|. (An exactly zero mean -- a shift with every tap out of range -- is
    robust: every product is an exact zero in any precision, so gy = 0.0001 exactly.)"""
    thr = GY_REL * float(part[..., 1].abs().mean())
    m = mean[:, 1].abs()
    return (m > 0) & (m <= thr)
