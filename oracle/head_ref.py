"""float64 restatements of the model head / tail, the BatchNorm finalizes, the SGD step and the
modality kernel (TEST INFRASTRUCTURE ONLY).

Plain torch / numpy, float64 inside: the reference ``tests/test_gpu_head_ref.py`` compares the
HIP kernels of head.hip, the two finalizes of bn.hip, optim.hip and ensemble.hip with, itself
pinned without a GPU against ``nn.BatchNorm1d``, autograd, ``torch.optim.SGD`` and
``oracle.ensemble_oracle`` (``tests/test_oracle_head.py``). Every function is written from the
contract in ``include/shiftgcn.h`` and the reference model lines it cites, not from the kernel
bodies.

Layout notes (shiftgcn.h, "Model head / tail of the training step"):

* the clip ``x`` is (N, C, T, V, M); the planes are (N*M, C, T, V);
* data_bn's features are in the reference order ``f = m*V*C + v*C + c``;
* the finalizes take partials (B, F, 2) in the LOCAL feature order and gamma / beta / running
  statistics / dgamma / dbeta in the REFERENCE order: ``perm_V = V > 0`` maps the local
  per-joint feature ``d*V + v`` to the reference feature ``v*D + d`` (D = F / V);
  ``perm_V = 0`` is the identity.
"""
from __future__ import annotations

import numpy as np
import torch

from . import stream_ref as sr

F64 = torch.float64
_d = sr._d


# --------------------------------------------------------------------------------------
# head: permute + data_bn (shift_gcn.py:194-198)
# --------------------------------------------------------------------------------------
def _feat(x):
    """(N, C, T, V, M) -> (N, M, V, C, T): data_bn's features (m, v, c), then t."""
    return _d(x).permute(0, 4, 3, 1, 2)


def _feat_planes(g, N, M):
    """planes (N*M, C, T, V) -> (N, M, V, C, T)."""
    NM, C, T, V = g.shape
    return _d(g).reshape(N, M, C, T, V).permute(0, 1, 4, 2, 3)


def _fvec(v, x):
    N, C, T, V, M = x.shape
    return _d(v).reshape(1, M, V, C, 1)


def head_moments(x):
    """``sgcn_head_moments``: (N, F, 2) {mean, M2} over t per (n, feature)."""
    N, C, T, V, M = x.shape
    xf = _feat(x).reshape(N, M * V * C, T)
    mean = xf.mean(2)
    return torch.stack((mean, ((xf - mean[:, :, None]) ** 2).sum(2)), -1)


def head_apply(x, scale, shift):
    """``sgcn_head_apply``: y[(n*M + m), c, t, v] = x[n, c, t, v, m]*scale[f] + shift[f]."""
    N, C, T, V, M = x.shape
    y = _feat(x) * _fvec(scale, x) + _fvec(shift, x)
    return y.permute(0, 1, 3, 4, 2).reshape(N * M, C, T, V)


def head_bwd_reduce(g, x, mean, invstd):
    """``sgcn_head_bwd_reduce``: (N, F, 2) {sum_t g, sum_t g*(x - mean[f])*invstd[f]}, g the
    plane-layout gradient."""
    N, C, T, V, M = x.shape
    gf = _feat_planes(g, N, M)
    xhat = (_feat(x) - _fvec(mean, x)) * _fvec(invstd, x)
    return torch.stack((gf.sum(-1), (gf * xhat).sum(-1)), -1).reshape(N, M * V * C, 2)


def head_bwd_apply(g, x, coef):
    """``sgcn_head_bwd_apply``: dx[n, c, t, v, m] = k1[f]*g + k2[f]*x + k3[f]."""
    N, C, T, V, M = x.shape
    k = _d(coef)
    dx = _fvec(k[0], x) * _feat_planes(g, N, M) + _fvec(k[1], x) * _feat(x) + _fvec(k[2], x)
    return dx.permute(0, 3, 4, 2, 1)


# --------------------------------------------------------------------------------------
# tail: global average pool (shift_gcn.py:211-214)
# --------------------------------------------------------------------------------------
def pool(x, N, M):
    """``sgcn_pool``: x.view(N, M, C, P).mean(3).mean(1), x (N*M, C, ...)."""
    C = x.shape[1]
    return _d(x).reshape(N, M, C, -1).mean(3).mean(1)


def pool_bwd_planes(dout, M, P):
    """``sgcn_pool_bwd_planes`` in float64: (N*M, C), dout[n][c] / M / P."""
    N, C = dout.shape
    return (_d(dout) / M / P)[:, None, :].expand(N, M, C).reshape(N * M, C)


def pool_bwd(dout, M, P):
    """``sgcn_pool_bwd`` in float64: (N*M, C, P), every plane at its plane value."""
    v = pool_bwd_planes(dout, M, P)
    return v[:, :, None].expand(v.shape[0], v.shape[1], P)


def pool_bwd_planes_f32(dout, M, P):
    """The exact float32 expression of the header: (dout * (1/M)) * (1/P) with float32
    reciprocals, as a numpy float32 (N*M, C) array."""
    d = dout.detach().cpu().numpy().astype(np.float32)
    N, C = d.shape
    rm = np.float32(1) / np.float32(M)
    rp = np.float32(1) / np.float32(P)
    v = ((d * rm).astype(np.float32) * rp).astype(np.float32)
    return np.broadcast_to(v[:, None, :], (N, M, C)).reshape(N * M, C).copy()


def pool_bwd_f32(dout, M, P):
    v = pool_bwd_planes_f32(dout, M, P)
    return np.broadcast_to(v[:, :, None], v.shape + (P,)).copy()


# --------------------------------------------------------------------------------------
# BatchNorm finalizes
# --------------------------------------------------------------------------------------
def to_local(v, perm_V):
    """A reference-order (F) vector in the local order: local d*V + v reads v*D + d."""
    return v if perm_V <= 0 else v.reshape(perm_V, -1).t().reshape(-1)


def to_ref(v, perm_V):
    """A local-order (F) vector in the reference order."""
    return v if perm_V <= 0 else v.reshape(-1, perm_V).t().reshape(-1)


def bn_finalize(part, B, n_part, gamma, beta, eps, momentum, running_mean, running_var,
                perm_V):
    """``sgcn_bn_finalize`` on (B, F, 2) partials {mean, M2} of n_part elements each.

    Returns (mean, invstd, scale, shift) in the local order, the new running mean and
    variance in the reference order (None without running statistics) and the element count
    B * n_part. gamma / beta None: 1 / 0. The running variance takes the unbiased batch
    variance; a single element (count 1) has no unbiased variance and takes the biased one."""
    part = _d(part)
    assert part.shape[0] == B
    F = part.shape[1]
    g = torch.ones(F, dtype=F64) if gamma is None else to_local(_d(gamma), perm_V)
    b = torch.zeros(F, dtype=F64) if beta is None else to_local(_d(beta), perm_V)
    mean, invstd, scale, shift = sr.bn_train_stats(part, n_part, g, b, eps)
    n = B * n_part
    m2 = part[..., 1].sum(0) + n_part * ((part[..., 0] - mean) ** 2).sum(0)
    unbiased = m2 / (n - 1) if n > 1 else m2 / n
    rm = rv = None
    if running_mean is not None:
        rm = (1 - momentum) * _d(running_mean) + momentum * to_ref(mean, perm_V)
        rv = (1 - momentum) * _d(running_var) + momentum * to_ref(unbiased, perm_V)
    return mean, invstd, scale, shift, rm, rv, n


def bn_bwd_finalize(part, n_total, perm_V, mean, invstd, gamma, accumulate_into=None,
                    batch_stats=True):
    """``sgcn_bn_bwd_finalize`` on (B, F, 2) partials {sum g, sum g*xhat}: (dgamma, dbeta) in
    the reference order, added to ``accumulate_into`` = (dgamma, dbeta) when given, and
    coef (3, F) in the local order; ``batch_stats`` False: k2 = k3 = 0 (a fixed affine map)."""
    F = part.shape[1]
    g = torch.ones(F, dtype=F64) if gamma is None else to_local(_d(gamma), perm_V)
    dg, db, coef = sr.bn_bwd_coef(part, n_total, mean, invstd, g)
    if not batch_stats:
        coef = torch.stack((coef[0], torch.zeros_like(coef[0]), torch.zeros_like(coef[0])))
    dg, db = to_ref(dg, perm_V), to_ref(db, perm_V)
    if accumulate_into is not None:
        dg, db = _d(accumulate_into[0]) + dg, _d(accumulate_into[1]) + db
    return dg, db, coef


# --------------------------------------------------------------------------------------
# optimizer (torch.optim.SGD, dampening 0)
# --------------------------------------------------------------------------------------
def sgd_step(p, g, buf, wd, lr, momentum, nesterov, first, scale=None):
    """``sgcn_sgd_step`` for one tensor, in the header's order: g = g*s (``scale`` given);
    d = g + wd*p (wd != 0); b = first ? d : momentum*b + d (momentum != 0); d = nesterov ?
    d + momentum*b : b; p = p - lr*d. Returns (p, buf, g) after the step; ``buf`` is returned
    unchanged (None allowed) when momentum == 0, and is not read when ``first``."""
    p, g = _d(p), _d(g)
    if scale is not None:
        g = g * float(scale)
    d = g
    if wd != 0:
        d = d + float(wd) * p
    if momentum != 0:
        b = d.clone() if first else float(momentum) * _d(buf) + d
        d = d + float(momentum) * b if nesterov else b
    else:
        b = buf
    return p - float(lr) * d, b, g


# --------------------------------------------------------------------------------------
# modalities (inference_pipeline.py:284-309 + the Model.forward head)
# --------------------------------------------------------------------------------------
def _planes(a):
    N, C, T, V, M = a.shape
    return a.permute(0, 4, 1, 2, 3).reshape(N * M, C, T, V)


def _modalities(j, parent):
    idx = torch.as_tensor(np.asarray(parent), dtype=torch.long)
    bone = j - j.index_select(3, idx)

    def motion(a):
        out = torch.zeros_like(a)
        out[:, :, :-1] = a[:, :, 1:] - a[:, :, :-1]
        return out

    return j, bone, motion(j), motion(bone)


def modalities(joint, parent, scale=None, shift=None, planes=False):
    """``sgcn_modalities`` in float64 for an arbitrary ``parent`` table (V): (joint, bone,
    joint_motion, bone_motion) in the (N, C, T, V, M) layout, or with ``planes`` in the
    (N*M, C, T, V) layout, there with data_bn's eval coefficients ``scale`` / ``shift``
    (4, M*V*C) applied when given."""
    outs = _modalities(_d(joint), parent)
    if not planes:
        assert scale is None and shift is None
        return outs
    N, C, T, V, M = joint.shape
    outs = [_planes(o) for o in outs]
    if scale is not None:
        def pv(v):      # (M*V*C) feature vector over the planes
            return _d(v).reshape(1, M, V, C).permute(0, 1, 3, 2).reshape(1, M, C, 1, V)
        outs = [(o.reshape(N, M, C, T, V) * pv(scale[k]) + pv(shift[k])).reshape(N * M, C, T, V)
                for k, o in enumerate(outs)]
    return tuple(outs)


def modalities_f32(joint, parent, planes=False):
    """The same differences evaluated in float32, in the header's order (bone_motion =
    bone[t+1] - bone[t] of the rounded bones): the bit-exact expectation without the affine."""
    outs = _modalities(joint.detach().cpu().float(), parent)
    return tuple(_planes(o).contiguous() if planes else o for o in outs)
