"""float64 torch restatements of the streaming kernels (TEST INFRASTRUCTURE ONLY).

Plain torch, device-agnostic, float64 inside: the reference the HIP BatchNorm-plane, gcn
gather / dx-finish, mask and shift-fused kernels are compared with
(``tests/test_gpu_stream_ref.py``), itself pinned without a GPU against ``nn.BatchNorm*d``,
autograd and the composed restatements (``tests/test_oracle_stream.py``). Every function
takes the logical tensors of the op of the same name in ``shiftgcn/ops.py`` and is written
from the contract in ``include/shiftgcn.h`` and the reference model lines it cites
(``model/shift_gcn.py``), not from the kernel bodies.

Layout notes (shiftgcn.h, "Training-mode BatchNorm"):

* planes are (B, C, T, V);
* ``per_joint = 3``: ``x`` is the Shift_gcn contraction output stored BEFORE its shift_out
  ("zu"); the logical tensor is ``z[c, t, w] = zu[c, t, (w - c) mod V]``
  (shift_gcn.py:114-118,136) and the per-joint features are in the local order
  ``f = c * V + w``;
* a mask ``m`` is (V, C): ``m[u, c]`` = ``tanh(Feature_Mask)[u, c] + 1``.

Every ReLU predicate is a select (``> 0 ? g : 0``, torch's ``threshold_backward``), never a
multiply: a non-finite gradient at a masked-out position gives 0.
"""
from __future__ import annotations

import numpy as np
import torch

from . import shift_oracle as so

F64 = torch.float64


def _d(t):
    return None if t is None else t.to(F64)


def _rot_index(C, V, sign, device):
    """(C, V) index table ``(v + sign * c) mod V``."""
    v = torch.arange(V, device=device)[None, :]
    c = torch.arange(C, device=device)[:, None]
    return (v + sign * c) % V


def _take_v(x, idx):
    B, C, T, V = x.shape
    return x.gather(3, idx.view(1, C, 1, V).expand(B, C, T, V))


def logical(zu):
    """``z[c, t, w] = zu[c, t, (w - c) mod V]``: the shift_out gather (shift_gcn.py:114-118)."""
    return _take_v(zu, _rot_index(zu.shape[1], zu.shape[3], -1, zu.device))


def prerotated(z):
    """Inverse of :func:`logical`: ``zu[c, t, v] = z[c, t, (v + c) mod V]``."""
    return _take_v(z, _rot_index(z.shape[1], z.shape[3], +1, z.device))


def _select(pred, g):
    return torch.where(pred > 0, g, torch.zeros_like(g))


def _pc(v, C):
    """per-channel (C) vector broadcast over (B, C, T, V)."""
    return _d(v).reshape(1, C, 1, 1)


def _pj(v, C, V):
    """per-joint local-order (C * V) vector broadcast over (B, C, T, V)."""
    return _d(v).reshape(1, C, 1, V)


def _full(dy, like):
    """A (B, C) per-plane gradient expanded over its planes; a full tensor unchanged."""
    dy = _d(dy)
    return dy[:, :, None, None].expand(like.shape) if dy.dim() == 2 else dy


# --------------------------------------------------------------------------------------
# BatchNorm plane kernels
# --------------------------------------------------------------------------------------
def moments(x, per_joint):
    """``sgcn_moments``: {mean, M2} partials, (B, C, 2) over each plane (per_joint 0) or
    (B, C, V, 2) over t per logical joint (per_joint 3)."""
    x = _d(x)
    if per_joint == 3:
        z = logical(x)
        mean = z.mean(2)
        return torch.stack((mean, ((z - mean[:, :, None]) ** 2).sum(2)), -1)
    if per_joint != 0:
        raise ValueError("per_joint must be 0 or 3")
    mean = x.mean((2, 3))
    return torch.stack((mean, ((x - mean[:, :, None, None]) ** 2).sum((2, 3))), -1)


def bn_train_stats(part, n_part, gamma, beta, eps):
    """``sgcn_bn_finalize`` arithmetic on (B, F, 2) partials of n_part elements each (local
    feature order throughout): batch mean, 1/sqrt(biased var + eps), scale, shift."""
    part = _d(part)
    B = part.shape[0]
    mean = part[..., 0].mean(0)
    m2 = part[..., 1].sum(0) + n_part * ((part[..., 0] - mean) ** 2).sum(0)
    invstd = (m2 / (B * n_part) + eps).rsqrt()
    scale = _d(gamma) * invstd
    return mean, invstd, scale, _d(beta) - mean * scale


def bn_bwd_coef(part, n_total, mean, invstd, gamma):
    """``sgcn_bn_bwd_finalize`` arithmetic on (B, F, 2) partials {sum g, sum g*xhat}:
    (dgamma, dbeta, coef (3, F)) with dx = k1*g + k2*x + k3 (training-mode BatchNorm)."""
    part = _d(part)
    sg, sgx = part[..., 0].sum(0), part[..., 1].sum(0)
    mean, invstd = _d(mean), _d(invstd)
    k1 = _d(gamma) * invstd
    k2 = -k1 * invstd * (sgx / n_total)
    k3 = -k1 * (sg / n_total) - k2 * mean
    return sgx, sg, torch.stack((k1, k2, k3))


def bn_apply(x, scale, shift, per_joint, r=None, rscale=None, rshift=None, relu=False,
             out_stats=False, gather_m=None):
    """``sgcn_bn_apply``: y = act(x*scale[f] + shift[f] + res) at the logical position.
    Returns y; (y, (B, C, 2) plane moments of y) with ``out_stats``; (y, gcn_gather(y, m))
    with ``gather_m``."""
    B, C, T, V = x.shape
    x = _d(x)
    if per_joint == 3:
        a = logical(x) * _pj(scale, C, V) + _pj(shift, C, V)
    elif per_joint == 0:
        a = x * _pc(scale, C) + _pc(shift, C)
    else:
        raise ValueError("per_joint must be 0 or 3")
    if r is not None:
        a = a + (_d(r) if rscale is None else _d(r) * _pc(rscale, C) + _pc(rshift, C))
    y = _select(a, a) if relu else a
    if gather_m is not None:
        return y, gcn_gather(y, gather_m)
    if out_stats:
        return y, moments(y, 0)
    return y


def _bn_bwd_g(dy, y, relu, dy_coef, like):
    B, C, T, V = like.shape
    g = _full(dy, like)
    if dy_coef is not None:
        k = _d(dy_coef)
        g = _pc(k[0], C) * g + _pc(k[1], C) * _d(y) + _pc(k[2], C)
    return _select(_d(y), g) if relu else g


def bn_bwd_reduce(dy, y, relu, x, mean, invstd, per_joint, r=None, rmean=None, rinvstd=None,
                  dy_coef=None):
    """``sgcn_bn_bwd_reduce``: part {sum g, sum g*xhat}, (B, C, 2) or (B, C, V, 2) (per_joint
    3, logical joints), and rpart (B, C, 2) for a BatchNorm2d residual input r (else None).
    ``dy`` (B, C) is one value per plane."""
    B, C, T, V = x.shape
    x = _d(x)
    g = _bn_bwd_g(dy, y, relu, dy_coef, x)
    if per_joint == 3:
        xhat = (logical(x) - _pj(mean, C, V)) * _pj(invstd, C, V)
        part = torch.stack((g.sum(2), (g * xhat).sum(2)), -1)
    elif per_joint == 0:
        xhat = (x - _pc(mean, C)) * _pc(invstd, C)
        part = torch.stack((g.sum((2, 3)), (g * xhat).sum((2, 3))), -1)
    else:
        raise ValueError("per_joint must be 0 or 3")
    rpart = None
    if r is not None:
        rhat = (_d(r) - _pc(rmean, C)) * _pc(rinvstd, C)
        rpart = torch.stack((g.sum((2, 3)), (g * rhat).sum((2, 3))), -1)
    return part, rpart


def bn_bwd_apply(dy, y, relu, x, coef, per_joint, r=None, rcoef=None, want_dr=False,
                 dy_coef=None):
    """``sgcn_bn_bwd_apply``: dx = k1*g + k2*x + k3 (per_joint 3: formed at the logical
    position, returned in the pre-rotation layout of x) and dr = g (``want_dr``) or
    rk1*g + rk2*r + rk3 (``rcoef``), else None."""
    B, C, T, V = x.shape
    x = _d(x)
    g = _bn_bwd_g(dy, y, relu, dy_coef, x)
    k = _d(coef)
    if per_joint == 3:
        dx = prerotated(_pj(k[0], C, V) * g + _pj(k[1], C, V) * logical(x) + _pj(k[2], C, V))
    elif per_joint == 0:
        dx = _pc(k[0], C) * g + _pc(k[1], C) * x + _pc(k[2], C)
    else:
        raise ValueError("per_joint must be 0 or 3")
    dr = None
    if rcoef is not None:
        q = _d(rcoef)
        dr = _pc(q[0], C) * g + _pc(q[1], C) * _d(r) + _pc(q[2], C)
    elif want_dr:
        dr = g
    return dx, dr


def bn_eval_coef(gamma, beta, running_mean, running_var, eps, perm_V=0):
    """``sgcn_bn_eval_coef``: (mean, invstd, scale, shift) from running statistics, in the
    local feature order (perm_V > 0: local f = d*V + v reads the module's feature v*D + d)."""
    def loc(t):
        t = _d(t)
        return t if perm_V <= 0 else t.view(perm_V, -1).t().reshape(-1)
    mean = loc(running_mean)
    invstd = (loc(running_var) + eps).rsqrt()
    scale = loc(gamma) * invstd
    return mean, invstd, scale, loc(beta) - mean * scale


# --------------------------------------------------------------------------------------
# Shift_gcn input side
# --------------------------------------------------------------------------------------
def mask_prep(mask):
    """``sgcn_mask_prep``: tanh(Feature_Mask) + 1 (shift_gcn.py:129)."""
    return torch.tanh(_d(mask)) + 1


def gcn_gather(x0, m):
    """``sgcn_gcn_gather``: xg[b,c,t,u] = x0[b,c,t,(u + c) mod V] * m[u, c]
    (shift_gcn.py:125-129)."""
    B, C, T, V = x0.shape
    return prerotated(_d(x0)) * _d(m).reshape(V, C).t().reshape(1, C, 1, V)


def gcn_dx_finish(dxt, x0, m, add1=None, add2=None, add2_mask=None, prev=None, mask_dx=False):
    """``sgcn_gcn_dx_finish``: (dx, dmask_part (B, C, V), prev_part (B, C, 2) or None).
    dx[b,c,t,v] = dxt[b,c,t,u]*m[u,c] + add1 + add2', u = (v - c) mod V, add2' = add2 or
    add2_mask > 0 ? add2 : 0 (``add2`` (B, C): one value per plane); dmask_part[b,c,u] =
    sum_t dxt[b,c,t,u] * x0[b,c,t,(u + c) mod V]; ``prev`` = (S, mean, invstd): the
    bn_bwd_reduce partials of g = x0 > 0 ? dx : 0 against xhat(S); ``mask_dx``: the dx
    returned is x0 > 0 ? dx : 0 (the sums are unchanged)."""
    B, C, T, V = dxt.shape
    dxt, x0 = _d(dxt), _d(x0)
    mcv = _d(m).reshape(V, C).t().reshape(1, C, 1, V)
    dx = logical(dxt * mcv)
    if add1 is not None:
        dx = dx + _d(add1)
    if add2 is not None:
        a2 = _full(add2, dxt)
        dx = dx + (a2 if add2_mask is None else _select(_d(add2_mask), a2))
    dmask_part = (dxt * prerotated(x0)).sum(2)
    prev_part = None
    if prev is not None:
        S, mean, invstd = prev
        g = _select(x0, dx)
        xhat = (_d(S) - _pc(mean, C)) * _pc(invstd, C)
        prev_part = torch.stack((g.sum((2, 3)), (g * xhat).sum((2, 3))), -1)
    if mask_dx:
        dx = _select(x0, dx)
    return dx, dmask_part, prev_part


def mask_grad_finalize(part, mask, accumulate=None):
    """``sgcn_mask_grad_finalize``: dmask[u, c] = (sum_b part[b, c, u]) * (1 - tanh(mask[u,
    c])^2), added to ``accumulate`` (the previous dmask) when given. Shape of ``mask``."""
    mask = _d(mask)
    V, C = mask.shape[-2:]
    s = _d(part).reshape(-1, C, V).sum(0).t()
    g = (s * (1 - torch.tanh(mask.reshape(V, C)) ** 2)).reshape(mask.shape)
    return g if accumulate is None else _d(accumulate) + g


# --------------------------------------------------------------------------------------
# shift-fused kernels: the operand formed here in float64, the shift by oracle.shift_oracle
# in float64 on the float32 position values the kernels use
# --------------------------------------------------------------------------------------
def _pos64(xpos, ypos, stride):
    """The kernels' float32 positions (ypos + 0.5 as a float32 add for stride != 1,
    shift.py:17-18), widened."""
    xp = xpos.detach().cpu().numpy().astype(np.float32)
    yp = so.effective_ypos(ypos.detach().cpu().numpy().astype(np.float32), stride)
    return xp.astype(np.float64), yp.astype(np.float64)


def _np(t):
    return t.detach().cpu().numpy()


def shift_fwd64(inp, xpos, ypos, stride):
    """oracle.shift_oracle.shift_forward of a float64 tensor, returned on its device."""
    xp, yp = _pos64(xpos, ypos, stride)
    return torch.from_numpy(so.shift_forward(_np(_d(inp)), xp, yp, stride)).to(inp.device)


def tshift_fwd_pre(z, xpos, ypos, stride, zscale, zshift, r, rscale, rshift, ascale, ashift):
    """``sgcn_tshift_fwd_pre``: shift(ascale[c]*H + ashift[c]), H = relu(z*zscale[c*W + w] +
    zshift[c*W + w] + res), z in the natural layout, res = r or r*rscale[c] + rshift[c]."""
    B, C, H, W = z.shape
    h = _d(z) * _pj(zscale, C, W) + _pj(zshift, C, W)
    h = h + (_d(r) if rscale is None else _d(r) * _pc(rscale, C) + _pc(rshift, C))
    h = _select(h, h)
    return shift_fwd64(h * _pc(ascale, C) + _pc(ashift, C), xpos, ypos, stride)


def tshift_fwd_tail(inp, xpos, ypos, stride, pscale, pshift, r=None, rscale=None, rshift=None,
                    gather_m=None):
    """``sgcn_tshift_fwd_tail``: out = relu(shift(inp)*pscale[c] + pshift[c] + res); returns
    (out, gcn_gather(out, gather_m) or None)."""
    C = inp.shape[1]
    a = shift_fwd64(inp, xpos, ypos, stride) * _pc(pscale, C) + _pc(pshift, C)
    if r is not None:
        a = a + (_d(r) if rscale is None else _d(r) * _pc(rscale, C) + _pc(rshift, C))
    out = _select(a, a)
    return out, (gcn_gather(out, gather_m) if gather_m is not None else None)


def tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos):
    """``sgcn_tshift_bwd_bnin`` (stride 1): gout = k1*(y > 0 ? dy : 0) + k2*s + k3 (``y``
    None: dy already masked; ``dy`` (B, C): one value per plane), gin = the shift's input
    gradient with the ReLU mask of ``inp``. Returns (gin, pos_part (B, C, 2): the
    pre-constraint per-plane position sums {x, y}, gx, gy: apply_shift_constraint of their
    batch mean, mean (C, 2): that batch mean)."""
    B, C, H, W = inp.shape
    k = _d(coef)
    g = _full(dy, inp)
    if y is not None:
        g = _select(_d(y), g)
    gout = _pc(k[0], C) * g + _pc(k[1], C) * _d(s) + _pc(k[2], C)
    xp, yp = _pos64(xpos, ypos, 1)
    dev = inp.device
    gin = torch.from_numpy(so.shift_bottom_backward(_np(gout), xp, yp, H, 1)).to(dev)
    gin = _select(_d(inp), gin)
    gxb, gyb = so.shift_position_backward(_np(_d(inp)), _np(gout), xp, yp, 1)
    part = torch.from_numpy(np.stack((gxb.sum((2, 3)), gyb.sum((2, 3))), -1)).to(dev)
    mean = part.mean(0)
    gx, gy = so.apply_shift_constraint(_np(mean[:, 0]), _np(mean[:, 1]))
    return gin, part, torch.from_numpy(gx).to(dev), torch.from_numpy(gy).to(dev), mean
