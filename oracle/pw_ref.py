"""float64 torch restatements of the pointwise-contraction entry points (TEST
INFRASTRUCTURE ONLY).

``sgcn_pw_fwd``, ``sgcn_pw_dw`` and ``sgcn_pw_fwd_tshift`` written from their contract in
``include/shiftgcn.h`` ("Pointwise (1x1) channel contraction with the joint-shift gathers
fused"), not from the kernel bodies: the reference ``tests/test_gpu_pw_ref.py`` compares the
MFMA kernels with, itself pinned without a GPU against ``F.conv2d`` + autograd and the
reference model's ``index_select`` gathers (``tests/test_oracle_pw.py``).

A plane operand is read and written through the header's addressing formula and nothing
else: element (b, ch, n = t*V + v) lives at

    ptr[b*bstride + ch*cstride + (t*tstride)*V + ((v + rsign*ch) mod V)]

evaluated here as an explicit int64 index tensor into the FLAT storage the operand's tensor
lives in (:meth:`Plane.index`). A :class:`Plane` takes its base offset and its batch and
channel strides from the tensor exactly as ``shiftgcn.ops.PlaneView`` does, so a sliced
tensor (a channel or batch slice of a larger one, its odd rows under ``tstride = 2``) is
addressed inside the larger storage, and the elements the formula does not name are simply
never touched.
"""
from __future__ import annotations

import torch

from . import stream_ref as sr

F64 = torch.float64


class Plane:
    """A plane operand: ``t`` (B, C', T', V) with unit stride over v (any batch / channel
    strides, any storage offset), the header's ``tstride`` and ``rsign``."""

    def __init__(self, t, tstride=1, rsign=0):
        if t.dim() != 4 or (t.shape[3] > 1 and t.stride(3) != 1):
            raise ValueError("plane operand: (B, C, T, V) with contiguous joints")
        self.t, self.tstride, self.rsign = t, int(tstride), int(rsign)
        self.offset, self.bstride, self.cstride = t.storage_offset(), t.stride(0), t.stride(1)

    def flat(self):
        """The whole storage behind ``t`` as a 1-D tensor (a view: writes reach ``t``)."""
        n = self.t.untyped_storage().nbytes() // self.t.element_size()
        return torch.as_strided(self.t, (n,), (1,), 0)

    def index(self, B, C, T, V):
        """(B, C, T, V) int64: the flat storage index of every logical element."""
        dev = self.t.device
        b = torch.arange(B, device=dev).view(B, 1, 1, 1)
        ch = torch.arange(C, device=dev).view(1, C, 1, 1)
        t = torch.arange(T, device=dev).view(1, 1, T, 1)
        v = torch.arange(V, device=dev).view(1, 1, 1, V)
        return (self.offset + b * self.bstride + ch * self.cstride + (t * self.tstride) * V +
                torch.remainder(v + self.rsign * ch, V))

    def read(self, B, C, T, V):
        """The logical (B, C, T, V) operand, float64."""
        return self.flat()[self.index(B, C, T, V)].to(F64)


def _weight(w, w_mcontig, M, K):
    """A[m][k] = w_mcontig ? w[k*M + m] : w[m*K + k]."""
    w = w.reshape(-1).to(F64)
    return w.view(K, M).t() if w_mcontig else w.view(M, K)


def _masked(x, mask, C, V):
    """X'(b, c, n) = X(b, c, n) * mask[v*C + c]."""
    if mask is None:
        return x
    return x * mask.reshape(-1).to(F64).view(V, C).t().reshape(1, C, 1, V)


def pw_fwd_ref(w, w_mcontig, bias, x: Plane, y: Plane, M, K, T, V, mask=None, relu=False,
               accumulate=False):
    """``sgcn_pw_fwd``: Y[b][m][out(n, m)] (+)= act(sum_k A[m][k] * X'(b, k, n) + bias[m]).

    Returns ``(flat, idx)``: a float64 copy of the whole storage behind ``y.t`` after the
    call (``accumulate``: the addition is to what the storage held; every element the
    formula does not name keeps its value) and the (B, M, T, V) index of the logical
    output elements in it (``flat[idx]`` is the logical output)."""
    B = x.t.shape[0]
    X = _masked(x.read(B, K, T, V), mask, K, V)
    val = torch.einsum("mk,bktv->bmtv", _weight(w, w_mcontig, M, K), X)
    if bias is not None:
        val = val + bias.to(F64).view(1, M, 1, 1)
    if relu:
        val = torch.where(val > 0, val, torch.zeros_like(val))
    idx = y.index(B, M, T, V)
    flat = y.flat().to(F64).clone()
    flat[idx] = flat[idx] + val if accumulate else val
    return flat, idx


def pw_dw_ref(g: Plane, x: Plane, M, Nc, T, V, mask=None, transpose=False, dw_old=None,
              dbias_old=None):
    """``sgcn_pw_dw``: dW[m][c] (+)= sum_{b, n} G(b, m, n) * X'(b, c, n), stored [c][m] when
    ``transpose``; dbias[m] (+)= sum_{b, n} G(b, m, n). ``dw_old`` / ``dbias_old``: the
    previous contents under dw_accumulate / dbias_accumulate (in the stored layout).
    Returns (dw, dbias), float64."""
    B = g.t.shape[0]
    G = g.read(B, M, T, V)
    X = _masked(x.read(B, Nc, T, V), mask, Nc, V)
    dw = torch.einsum("bmtv,bctv->mc", G, X)
    if transpose:
        dw = dw.t()
    db = G.sum((0, 2, 3))
    if dw_old is not None:
        dw = dw + dw_old.to(F64).view(dw.shape)
    if dbias_old is not None:
        db = db + dbias_old.to(F64)
    return dw.contiguous(), db


def pw_fwd_tshift_ref(w, bias, x: Plane, xpos, ypos, scale, shift, y: Plane, M, K, T, V,
                      relu=False):
    """``sgcn_pw_fwd_tshift``: Y[b][m][n] = act(sum_k w[m*K + k] * S_k(b, n) + bias[m]),
    S_k = shift_k(in_scale[k] * X[b][k] + in_shift[k]) (stride-1 temporal shift by
    ``oracle.shift_oracle`` in float64 on the float32 positions, as ``stream_ref``).
    Returns ``(flat, idx, S)``: as :func:`pw_fwd_ref`, and the side output S (B, K, T, V)."""
    B = x.t.shape[0]
    X = x.read(B, K, T, V)
    if scale is not None:
        X = X * scale.to(F64).view(1, K, 1, 1) + shift.to(F64).view(1, K, 1, 1)
    S = sr.shift_fwd64(X, xpos, ypos, 1).contiguous()
    flat, idx = pw_fwd_ref(w, False, bias, Plane(S), y, M, K, T, V, relu=relu)
    return flat, idx, S
