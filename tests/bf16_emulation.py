"""The float64 oracle with the device's bf16 rounding points (TEST INFRASTRUCTURE ONLY).

``emulate_bf16(module)`` takes an oracle module (oracle/model_oracle.py: a block, a unit or
a whole Model, in eval mode and float64) and gives its Shift_gcn, Shift_tcn and residual tcn
sub-modules forwards that compute what the eval-mode "bf16" precision computes on the device
(shiftgcn.fused._eval_pw_fwd), with everything else in float64:

* at every contraction with K >= 32 input channels both operands are rounded to bf16 (round
  to nearest even): the weight, after the eval-mode BatchNorm that follows the conv is folded
  into it where the device folds (Shift_gcn.down and the residual tcn, fused.folded_conv_bn),
  and the input operand, for Shift_gcn after the shift_in gather and the mask multiply;
* contractions with K < 32 (l1's gcn Linear and down conv on the raw coordinates) are not
  rounded;
* BatchNorms, shifts, biases, ReLUs, residual adds, the head and fc are float64.

The oracle's classes are not edited: the forwards are bound on the instances given here.
"""
from __future__ import annotations

import types

import torch
from torch import nn

from oracle import model_oracle as mo

MIN_K = 32    # shiftgcn.fused.BF16_MIN_K


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _contract(w, x):
    """sum_k w[m][k] * x[b][k][t][v], both rounded to bf16 when K >= MIN_K."""
    if w.shape[1] >= MIN_K:
        w, x = round_bf16(w), round_bf16(x)
    return torch.einsum("mk,bktv->bmtv", w, x)


def _folded(conv, bn, x, stride=1):
    """Eval-mode conv (1 x 1, time stride) -> BatchNorm as ONE contraction, the weight rounded
    after folding."""
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    t = bn.bias - bn.running_mean * s
    w = conv.weight[:, :, 0, 0] * s[:, None]
    b = conv.bias * s + t
    return _contract(w, x[:, :, ::stride]) + b.view(1, -1, 1, 1)


def _gcn_forward(self, x0):
    n, c, t, v = x0.size()
    x = x0.permute(0, 2, 3, 1).contiguous().view(n * t, v * c)
    x = torch.index_select(x, 1, self.shift_in).view(n * t, v, c)
    x = x * (torch.tanh(self.Feature_Mask) + 1)
    w = self.Linear_weight
    if c >= MIN_K:
        x, w = round_bf16(x), round_bf16(w)          # the operand: after the mask multiply
    x = torch.einsum("nwc,cd->nwd", x, w).contiguous()
    x = x + self.Linear_bias
    x = torch.index_select(x.view(n * t, -1), 1, self.shift_out)
    x = self.bn(x)
    x = x.view(n, t, v, self.out_channels).permute(0, 3, 1, 2)
    if isinstance(self.down, nn.Sequential):
        x = x + _folded(self.down[0], self.down[1], x0)
    else:
        x = x + x0
    return self.relu(x)


def _tcn_forward(self, x):
    x = self.shift_in(self.bn(x))
    tl = self.temporal_linear
    x = _contract(tl.weight[:, :, 0, 0], x) + tl.bias.view(1, -1, 1, 1)
    x = self.shift_out(torch.relu(x))
    return self.bn2(x)


def _residual_forward(self, x):
    assert self.conv.kernel_size == (1, 1)
    return _folded(self.conv, self.bn, x, self.conv.stride[0])


def emulate_bf16(module):
    """Bind the rounding forwards on every Shift_gcn / Shift_tcn / tcn of ``module`` (in
    place; pass a copy to keep the plain oracle) and return it."""
    assert not module.training
    for m in module.modules():
        if isinstance(m, mo.Shift_gcn):
            m.forward = types.MethodType(_gcn_forward, m)
        elif isinstance(m, mo.Shift_tcn):
            m.forward = types.MethodType(_tcn_forward, m)
        elif isinstance(m, mo.tcn):
            m.forward = types.MethodType(_residual_forward, m)
    return module
