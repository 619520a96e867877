"""float64 restatements of the temporal-shift entry points the training step runs (TEST
INFRASTRUCTURE ONLY): sgcn_tshift_fwd, sgcn_tshift_bwd, sgcn_tshift_bwd_gbn,
sgcn_tshift_pos_finalize and sgcn_bn_bwd_finalize_gbn.

The reference ``tests/test_gpu_tshift_ref.py`` compares the HIP kernels with, itself pinned
without a GPU (``tests/test_oracle_tshift.py``) against ``oracle.torch_shift``, autograd and
``nn.BatchNorm*d`` in double. Every function is written from the contract in
``include/shiftgcn.h``, not from the kernel bodies: the shift itself is
``oracle.shift_oracle`` evaluated in float64 on the float32 position values the kernels use
(``stream_ref._pos64``), the fused options are formed around it in float64.

* the affine ``scale[c]*x + shift[c]`` applies to in-range taps only: shifting the
  pre-affined tensor, whose out-of-range taps the shift fills with 0 (not ``shift[c]``);
* every ``> 0`` predicate is a select (``stream_ref._select``), never a multiply;
* ``z`` of the GBN form is the gcn contraction output stored BEFORE its shift_out: the
  logical joint w of channel c sits at ``(w - c) mod W`` (``stream_ref.logical``).

All arguments are the logical CPU or device tensors; results are float64 on ``inp``'s device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import shift_oracle as so
from . import stream_ref as sr

F64 = torch.float64


def _affined(inp, scale, shift):
    """The tensor whose taps the shift reads: ``scale[c]*inp + shift[c]`` or ``inp``."""
    x = sr._d(inp)
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift come together")
    if scale is None:
        return x
    C = inp.shape[1]
    return x * sr._pc(scale, C) + sr._pc(shift, C)


def _from(a, like):
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.device)


def tshift_fwd(inp, xpos, ypos, stride, scale=None, shift=None):
    """``sgcn_tshift_fwd`` (``ypos`` the raw parameter): (out (B, C, H // stride, W), stats
    (B, C, 2) = {mean, M2} of each output plane; None for an empty output)."""
    xp, yp = sr._pos64(xpos, ypos, stride)
    out = _from(so.shift_forward(sr._np(_affined(inp, scale, shift)), xp, yp, stride), inp)
    return out, (sr.moments(out, 0) if out.numel() else None)


def pos_finalize(part):
    """``sgcn_tshift_pos_finalize`` of (B, C, 2) partials: (gx, gy, mean (C, 2)), the fp64
    batch mean followed by applyShiftConstraint."""
    mean = sr._d(part).mean(0)
    gx, gy = so.apply_shift_constraint(sr._np(mean[:, 0]), sr._np(mean[:, 1]))
    return _from(gx, part), _from(gy, part), mean


def tshift_bwd(gout, inp, xpos, ypos, stride, scale=None, shift=None, relu_mask=False,
               bn_mean=None, bn_invstd=None):
    """``sgcn_tshift_bwd``: (gin, pos_part (B, C, 2), bn_part (B, C, 2) or None, gx, gy, mean
    (C, 2)). gin = the reversed shift of gout, 0 where ``inp <= 0`` under ``relu_mask``;
    pos_part = the per-plane sums of the position products {x, y} on the affine taps; bn_part
    = {sum gin, sum gin*(inp - bn_mean[c])*bn_invstd[c]}; gx, gy = :func:`pos_finalize`."""
    B, C, H, W = inp.shape
    xp, yp = sr._pos64(xpos, ypos, stride)
    g64 = sr._np(sr._d(gout))
    gin = _from(so.shift_bottom_backward(g64, xp, yp, H, stride), inp)
    if relu_mask:
        gin = sr._select(sr._d(inp), gin)
    gxb, gyb = so.shift_position_backward(sr._np(_affined(inp, scale, shift)), g64, xp, yp,
                                          stride)
    part = _from(np.stack((gxb.sum((2, 3)), gyb.sum((2, 3))), -1), inp)
    bn_part = None
    if bn_mean is not None:
        xhat = (sr._d(inp) - sr._pc(bn_mean, C)) * sr._pc(bn_invstd, C)
        bn_part = torch.stack((gin.sum((2, 3)), (gin * xhat).sum((2, 3))), -1)
    gx, gy, mean = pos_finalize(part)
    return gin, part, bn_part, gx, gy, mean


def _six(act, gin, hc, xh, dims):
    """{sum gin, sum (in - mu), sum 1, sum gin*xh, sum (in - mu)*xh, sum xh} where ``act``."""
    zero = torch.zeros_like(gin)
    kinds = (gin, hc, torch.ones_like(gin), gin * xh, hc * xh, xh)
    return torch.stack([torch.where(act, k, zero).sum(dims) for k in kinds])


def tshift_bwd_gbn(gout, inp, xpos, ypos, scale, shift, bn_mean, bn_invstd, z, z_mean,
                   z_invstd, d=None, d_mean=None, d_invstd=None):
    """``sgcn_tshift_bwd_gbn``: :func:`tshift_bwd` (stride 1, affine, bn_part, no ReLU mask)
    + z_part (6, B, C, W): the six sums over t where ``inp > 0`` per (plane, logical joint),
    zh = (z_logical - z_mean[c*W + w]) * z_invstd[c*W + w]; + d_part (6, B, C) (``d`` given,
    else None): the same sums over the plane with dh = (d - d_mean[c]) * d_invstd[c], d in
    the natural layout."""
    B, C, H, W = inp.shape
    res = tshift_bwd(gout, inp, xpos, ypos, 1, scale, shift, False, bn_mean, bn_invstd)
    gin, x = res[0], sr._d(inp)
    act = x > 0
    hc = x - sr._pc(bn_mean, C)
    zh = (sr.logical(sr._d(z)) - sr._pj(z_mean, C, W)) * sr._pj(z_invstd, C, W)
    z_part = _six(act, gin, hc, zh, 2)
    d_part = None
    if d is not None:
        dh = (sr._d(d) - sr._pc(d_mean, C)) * sr._pc(d_invstd, C)
        d_part = _six(act, gin, hc, dh, (2, 3))
    return res + (z_part, d_part)


def bn_bwd_finalize_gbn(part6, n_total, dy_coef, dy_mean, mean, invstd, gamma):
    """``sgcn_bn_bwd_finalize_gbn`` on (6, B, C, V) sums (V = 1: the down BatchNorm's (6, B,
    C)): g = k1*gin + k2*(in - mu) + (k3 + k2*mu) with dy_coef = (3, C) {k1, k2, k3} and
    dy_mean = mu (C), so sum g = k1*S0 + k2*S1 + (k3 + k2*mu)*S2 and sum g*xhat likewise of
    S3..S5; then (dgamma, dbeta, coef (3, C*V)) as ``stream_ref.bn_bwd_coef``. ``mean``,
    ``invstd``, ``gamma`` and the results are in the local feature order c*V + v."""
    p = sr._d(part6)
    if p.dim() == 3:
        p = p[..., None]
    _, B, C, V = p.shape
    k = sr._d(dy_coef)
    k1, k2 = k[0].reshape(1, C, 1), k[1].reshape(1, C, 1)
    k3 = (k[2] + k[1] * sr._d(dy_mean)).reshape(1, C, 1)
    sg = k1 * p[0] + k2 * p[1] + k3 * p[2]
    sgx = k1 * p[3] + k2 * p[4] + k3 * p[5]
    part = torch.stack((sg, sgx), -1).reshape(B, C * V, 2)
    return sr.bn_bwd_coef(part, n_total, mean, invstd, gamma)
