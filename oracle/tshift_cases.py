"""Shape table of the temporal-shift reference tests, and Python mirrors of the launch choosers
of sgcn_tshift_fwd, sgcn_tshift_bwd and sgcn_tshift_bwd_gbn (TEST INFRASTRUCTURE ONLY).

``tests/test_gpu_tshift_ref.py`` runs the three entry points over :data:`TABLE` at stride 1
and 2 (+ :data:`FWD_ONLY`); ``tests/test_oracle_tshift.py`` checks, without a GPU, that
those planes reach every launch form a plane CAN reach, by enumerating all planes through
the mirrors below. Each mirror restates one host function of
``shift-gcn_amd/csrc/launch_forms.hpp`` (``tshift_fwd_form``, ``bwd_form``, ``gbn_form``;
``tests/test_launch_forms.py`` compares them with that header on every plane); the choosers
shared with the shift-fused entry points come from ``oracle.stream_cases``. Every form stands for
the 4 (forward: affine x stats) or 8 (backward: affine x relu_mask x bn_part) template
instances behind it, which the GPU test runs on every plane.
"""
from __future__ import annotations

from . import stream_cases as sc
from .stream_cases import pad_fwd_lpt, pad_lds_fits, pick_lpt, ra_lpt

K_THREADS = 256          # launch_forms.hpp kThreads (the global-tap kernels)
K_BWD_THREADS = 512      # launch_forms.hpp kBwdThreads
K_RA_SPLIT256 = 8192     # launch_forms.hpp kRaSplit256
GBD_SPLIT = True         # launch_forms.hpp SGCN_GBD_SPLIT


def pick_ept(n):
    """launch_forms.hpp ``pick_ept``."""
    per = -(-n // K_THREADS)
    return 8 if per <= 8 else 16 if per <= 16 else 32


def fwd_form(H, W, stride):
    """Launch form of sgcn_tshift_fwd: ("pad", threads, per-thread) (tshift_fwd_pad_kernel),
    ("lds", threads, per-thread) (tshift_fwd_lds_kernel), ("global", per-thread, loops)
    (tshift_fwd_kernel; ``loops``: more than one pass of per-thread x 256 outputs) or "empty"
    (H // stride == 0: nothing is launched)."""
    Ho, n = H // stride, H * W
    if Ho == 0:
        return "empty"
    if n <= sc.K_FWD_LDS_MAX2:
        nt = 256 if n <= sc.K_FWD_LDS_MAX else 512
        lpt = pad_fwd_lpt(H, W, nt)
        if lpt:
            return ("pad", nt, lpt)
        if n <= sc.K_FWD_LDS_MAX:
            return ("lds", 256, pick_lpt(n, 256))
        return ("lds", 512, 32)
    ept = pick_ept(Ho * W)
    return ("global", ept, Ho * W > ept * K_THREADS)


def bwd_form(H, W, stride):
    """Launch form of sgcn_tshift_bwd (H >= 1): ("ra", threads, per-thread)
    (tshift_bwd_ra_kernel, stride 1), ("s2", per-thread, joint-aligned) (tshift_bwd_s2_kernel,
    stride 2) or ("global", stride, per-thread, loops) (tshift_bwd_kernel)."""
    n = H * W
    if stride == 1:
        nt = 256 if n <= K_RA_SPLIT256 and ra_lpt(n, 256, W) else K_BWD_THREADS
        lpt = ra_lpt(n, nt, W)
        if lpt and pad_lds_fits(H, W):
            return ("ra", nt, lpt)
    elif stride == 2:
        both = (H + H // 2) * W
        if both <= sc.K_BWD_LDS_MAX:
            return ("s2", pick_lpt(both, K_BWD_THREADS), W <= 64)
    else:
        raise ValueError("the backward takes stride 1 or 2")
    ept = pick_ept(n)
    return ("global", stride, ept, n > ept * K_THREADS)


def gbn_form(H, W, down):
    """Launch form of sgcn_tshift_bwd_gbn: ("ra", threads, per-thread, down) or "refuse"
    (SGCN_EINVAL). With the down BatchNorm's sums a plane that would hold more than 24
    elements per thread on 256 threads takes 512 (SGCN_GBD_SPLIT)."""
    n = H * W
    if W > 64 or n > sc.K_BWD_LDS_MAX:
        return "refuse"
    l256 = ra_lpt(n, 256, W) if n <= K_RA_SPLIT256 else 0
    nt = 256 if l256 and not (GBD_SPLIT and down and l256 > 24) else K_BWD_THREADS
    lpt = ra_lpt(n, nt, W)
    lds = max(sc.ra_pad_floats(H, W) + 1, 6 * nt) * 4      # ra_lds_bytes with GBN
    if lpt == 0 or lds > sc.K_LDS_BYTES:
        return "refuse"
    return ("ra", nt, lpt, bool(down))


def reachable(form, v_max=130, n_max=sc.K_FWD_LDS_MAX2 + 2 * 256):
    """Every value ``form(H, W)`` takes over the planes W <= v_max, H * W <= n_max (past the
    largest threshold nothing new can appear), "refuse" excluded."""
    out = set()
    for W in range(1, v_max + 1):
        for H in range(1, n_max // W + 2):
            f = form(H, W)
            if f != "refuse":
                out.add(f)
    return out


# --------------------------------------------------------------------------------------
# the shape table: (B, C, H, W), every plane run at stride 1 and at stride 2
# --------------------------------------------------------------------------------------
EXTRA = [
    (1, 2, 656, 25),     # 16,400 floats: the first global-tap forward, two passes
    (1, 2, 497, 33),     # stride 2: global forward in one pass (248 x 33 = 8,184 outputs)
    (1, 2, 85, 65),      # stride 2: s2 x 32 without the joint-aligned walk (W > 64)
    (1, 2, 169, 33),     # GBN with a down conv: 512 x 12
    (1, 2, 21, 25),      # odd H (stream_cases.STRIDE2): the last input row feeds no output
    (1, 2, 301, 25),     # odd H, stride 2: s2 x 32 joint-aligned
]


def _planes(shape):
    """Two-channel shapes take B = 2. One of the eight position entries puts every tap out of
    range, so a variant of a (1, 2, H, W) case would leave ONE non-zero plane sum per kind,
    and the SUM bar (relative to the largest sum of the vector) would then test how far that
    one sum of H * W zero-mean products happens to cancel: an fp32 sum of n terms carries
    ~6e-8 * sqrt(n) * rms, 1e-5 of the sum only while |sum| > 0.006 * sqrt(n) * rms, which
    one sum in sixty misses. With B = 2 every vector holds at least two live sums.

    Measured at B = 1 on an MI355X (error / the one live |reference sum| of the vector; all
    in the variant with the dead channel): position y sum 4.1e-6 / 0.307 at (320, 25) stride
    2 and 1.05e-5 / 0.0365 at (641, 25) (16,025 products of unit scale: a sum of natural
    size ~100 cancelled to 0.04, and 10 x SUM of it, the cap of the fp32-torch allowance, is
    3.7e-6: below what any fp32 evaluation of that sum achieves); position x sum 7.2e-6 /
    0.377 at (497, 33); bn_part[1] 2.7e-6 / 0.0754 at (325, 25) and 3.6e-6 / 0.00815 at
    (240, 33). Every error is an absolute 3e-6 .. 1e-5 on 8,000 .. 16,000 unit-scale terms;
    the same kernels hold <= 0.37 of SUM on the same planes once a second live sum sets the
    vector's scale."""
    B, C, H, W = shape
    return (2 if C == 2 else B, C, H, W)


TABLE = [_planes(s) for s in sc.SHIFT_TABLE + EXTRA]

# forward only: stride 3 (the header accepts stride >= 1; the backward takes 1 or 2)
FWD_ONLY = [((2, 3, 22, 25), 3)]

EMPTY = (2, 2, 1, 25)    # at stride 2: H // stride == 0
assert EMPTY in TABLE

FWD_CASES = [(s, st) for s in TABLE for st in (1, 2)] + FWD_ONLY
BWD_CASES = [(s, st) for s in TABLE for st in (1, 2)]
GBN_SHAPES = list(TABLE)

# float64 entry points: a ragged 256 x 8 plane, the MediaPipe plane, odd H at stride 2
F64_CASES = [((2, 5, 7, 25), 1), ((1, 3, 300, 33), 1), ((2, 2, 21, 25), 2)]
assert all(s in TABLE for s, _ in F64_CASES)

n_variants = sc.n_variants


# --------------------------------------------------------------------------------------
# deterministic inputs (float32, CPU); per-channel vectors are distinct across channels
# --------------------------------------------------------------------------------------
def _seed(variant, stride):
    return 1000 + 100 * variant + 30 * stride


def fwd_inputs(shape, variant, stride):
    """(inp, xpos, ypos, scale, shift) of one sgcn_tshift_fwd case."""
    B, C, H, W = shape
    sd = _seed(variant, stride)
    xpos, ypos = sc.positions(C, H, variant)
    return (sc.t(shape, sd + 1, 1.0, 0.3), xpos, ypos, sc.t((C,), sd + 2, 0.5, 1.0),
            sc.t((C,), sd + 3, 0.3))


def bwd_inputs(shape, variant, stride):
    """dict of one sgcn_tshift_bwd / sgcn_tshift_bwd_gbn case: gout, inp (feeds the ``> 0``
    predicates: ``stream_cases.act``), xpos, ypos, scale, shift, bn_mean, bn_invstd and, for
    GBN, z, z_mean, z_invstd (C * W, local order), d, d_mean, d_invstd."""
    B, C, H, W = shape
    sd = _seed(variant, stride)
    xpos, ypos = sc.positions(C, H, variant)
    return dict(
        gout=sc.t((B, C, H // stride, W), sd + 4), inp=sc.act(shape, sd + 5), xpos=xpos,
        ypos=ypos, scale=sc.t((C,), sd + 6, 0.5, 1.0), shift=sc.t((C,), sd + 7, 0.3),
        bn_mean=sc.t((C,), sd + 8, 0.3), bn_invstd=sc.t((C,), sd + 9, 0.4, 1.0),
        z=sc.t(shape, sd + 10, 2.0, 0.3), z_mean=sc.t((C * W,), sd + 11, 0.3),
        z_invstd=sc.t((C * W,), sd + 12, 0.4, 1.0), d=sc.t(shape, sd + 13, 1.5, -0.2),
        d_mean=sc.t((C,), sd + 14, 0.3), d_invstd=sc.t((C,), sd + 15, 0.4, 1.0))


def finalize_inputs(B, C):
    """Hand-made (B, C, 2) float32 partials of sgcn_tshift_pos_finalize: random channels
    (y sums offset by +-1), and (where C allows) channel 0 all-zero y sums (gy = 0.0001,
    gx = 0), channel 1 large values of both signs that cancel to a small non-zero mean
    (+-2^10 pairs plus 0.5 per plane on even B, one unpaired 3.0 more on odd B), channel 2
    negative throughout. The finalized outputs carry only the sign of the batch mean, and the
    test keeps a channel only while |mean| > GY_REL x mean |partial| (stream_cases.gy_unsafe):
    such a mean survives any merge order and precision (an fp32 merge of 70 partials errs by
    ~4e-6 relative), so these inputs check the batch slicing, the four channels per workgroup
    and the dr == 0 branch, not the width of the accumulator."""
    import torch
    part = sc.t((B, C, 2), 7000 + 10 * B + C, 3.0)
    part[..., 1] += 1.0 - 2.0 * (torch.arange(C) % 2)     # batch means away from 0, both signs
    part[:, 0, 1] = 0.0
    if C > 1:
        big = torch.full((B,), float(2 ** 10))
        big[1::2] = -float(2 ** 10)
        if B % 2:
            big[-1] = 3.0
        part[:, 1, 1] = big + 0.5
        part[:, 1, 0] = -big
    if C > 2:
        part[:, 2, 1] = -part[:, 2, 1].abs() - 0.25
    return part
