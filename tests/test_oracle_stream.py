"""Pin the float64 restatements of the streaming kernels (oracle/stream_ref.py) without a
GPU: against nn.BatchNorm2d / BatchNorm1d and autograd in double, against the reference's
index_select gather (oracle/model_oracle.py), and against their own compositions; and check
that the shape table of tests/test_gpu_stream_ref.py reaches every launch form a plane can
reach (oracle/stream_cases.py mirrors the launch choosers)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import model_oracle as mo
from oracle import shift_oracle as so
from oracle import stream_cases as sc
from oracle import stream_ref as sr

F64 = torch.float64
TOL = 1e-12


def _t(shape, seed, scale=1.0, offset=0.0):
    return sc.t(shape, seed, scale, offset).double()


def _close(a, b, tol=TOL):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= tol * (float(b.abs().max()) + 1e-300)


def _loc(v, C, V):
    """module feature order (v*C + c) -> local order (c*V + v)"""
    return v.reshape(V, C).t().reshape(-1)


def _bn2d(C, seed):
    bn = nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(_t((C,), seed, 0.4, 1.0))
        bn.bias.copy_(_t((C,), seed + 1, 0.3))
    return bn


# --------------------------------------------------------------------------------------
# BatchNorm: forward + autograd
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", ["none", "identity", "bn"])
@pytest.mark.parametrize("relu", [True, False])
def test_bn2d_forward_backward(res, relu):
    B, C, T, V = 3, 5, 7, 6
    shape = (B, C, T, V)
    x = _t(shape, 1, 2.0, 0.3).requires_grad_(True)
    r = _t(shape, 2).requires_grad_(True) if res != "none" else None
    dy = _t(shape, 3)
    bn, rbn = _bn2d(C, 4), _bn2d(C, 6)
    a = bn(x)
    if res == "identity":
        a = a + r
    if res == "bn":
        a = a + rbn(r)
    y_t = torch.relu(a) if relu else a
    y_t.backward(dy)

    n = T * V
    mean, invstd, scale, shift = sr.bn_train_stats(sr.moments(x, 0), n, bn.weight, bn.bias, bn.eps)
    assert _close(mean, x.detach().mean((0, 2, 3)))
    assert _close(invstd, (x.detach().var((0, 2, 3), unbiased=False) + bn.eps).rsqrt())
    rs = None
    if res == "bn":
        rs = sr.bn_train_stats(sr.moments(r, 0), n, rbn.weight, rbn.bias, rbn.eps)
    y, ys = sr.bn_apply(x, scale, shift, 0, r, rs[2] if rs else None, rs[3] if rs else None,
                        relu=relu, out_stats=True)
    assert _close(y, y_t.detach())
    assert _close(ys[..., 0], y_t.detach().mean((2, 3)))
    assert _close(ys[..., 1], y_t.detach().var((2, 3), unbiased=False) * n)

    yy = y if relu else None
    part, rpart = sr.bn_bwd_reduce(dy, yy, relu, x, mean, invstd, 0, r if rs else None,
                                   rs[0] if rs else None, rs[1] if rs else None)
    dgamma, dbeta, coef = sr.bn_bwd_coef(part, B * n, mean, invstd, bn.weight)
    assert _close(dgamma, bn.weight.grad) and _close(dbeta, bn.bias.grad)
    rcoef = None
    if rs:
        rdg, rdb, rcoef = sr.bn_bwd_coef(rpart, B * n, rs[0], rs[1], rbn.weight)
        assert _close(rdg, rbn.weight.grad) and _close(rdb, rbn.bias.grad)
    dx, dr = sr.bn_bwd_apply(dy, yy, relu, x, coef, 0, r if rs else None, rcoef,
                             want_dr=res == "identity")
    assert _close(dx, x.grad)
    if res == "none":
        assert dr is None
    else:
        assert _close(dr, r.grad)
    # a pre-masked dy (relu = 0, y = None) and a per-plane dy are the same sums
    if relu:
        pre = torch.where(y > 0, dy, torch.zeros_like(dy))
        p2, _ = sr.bn_bwd_reduce(pre, None, False, x, mean, invstd, 0)
        assert _close(p2, part)
    dyp = _t((B, C), 8)
    full = dyp[:, :, None, None].expand(shape)
    pa, _ = sr.bn_bwd_reduce(dyp, yy, relu, x, mean, invstd, 0)
    pb, _ = sr.bn_bwd_reduce(full, yy, relu, x, mean, invstd, 0)
    assert _close(pa, pb, 0.0)


@pytest.mark.parametrize("res", ["none", "identity", "bn"])
@pytest.mark.parametrize("C", [5, 9])     # C > V: the rotation wraps
def test_bn1d_per_joint_with_following_bn(res, C):
    """per_joint = 3 on the pre-shift_out tensor: Shift_gcn.bn = BatchNorm1d(V*C) over the
    logical z (shift_gcn.py:135-141), + down(x0), ReLU, then Shift_tcn.bn (BatchNorm2d) whose
    input gradient enters the backward as dy_coef."""
    B, T, V = 3, 4, 7
    shape = (B, C, T, V)
    zu = _t(shape, 11, 2.0, 0.3).requires_grad_(True)
    r = _t(shape, 12).requires_grad_(True) if res != "none" else None
    dA = _t(shape, 13)
    bn1 = nn.BatchNorm1d(V * C).double()
    with torch.no_grad():
        bn1.weight.copy_(_t((V * C,), 14, 0.4, 1.0))
        bn1.bias.copy_(_t((V * C,), 15, 0.3))
    rbn, bn2 = _bn2d(C, 16), _bn2d(C, 18)
    z = sr.logical(zu)                                         # (B, C, T, V)
    zf = z.permute(0, 2, 3, 1).reshape(B * T, V * C)           # feature v*C + c
    a = bn1(zf).view(B, T, V, C).permute(0, 3, 1, 2)
    if res == "identity":
        a = a + r
    if res == "bn":
        a = a + rbn(r)
    h_t = torch.relu(a)
    bn2(h_t).backward(dA)

    g1, b1 = _loc(bn1.weight.detach(), C, V), _loc(bn1.bias.detach(), C, V)
    part = sr.moments(zu, 3)
    assert part.shape == (B, C, V, 2)
    mean, invstd, scale, shift = sr.bn_train_stats(part.reshape(B, C * V, 2), T, g1, b1, bn1.eps)
    zd = z.detach()
    assert _close(mean.view(C, V), zd.mean((0, 2)))
    rs = None
    if res == "bn":
        rs = sr.bn_train_stats(sr.moments(r, 0), T * V, rbn.weight, rbn.bias, rbn.eps)
    h = sr.bn_apply(zu, scale, shift, 3, r, rs[2] if rs else None, rs[3] if rs else None,
                    relu=True)
    assert _close(h, h_t.detach())
    # the following BatchNorm2d: statistics of h, then its backward coefficients
    m2, i2, _, _ = sr.bn_train_stats(sr.moments(h, 0), T * V, bn2.weight, bn2.bias, bn2.eps)
    p2, _ = sr.bn_bwd_reduce(dA, None, False, h, m2, i2, 0)
    dg2, db2, k = sr.bn_bwd_coef(p2, B * T * V, m2, i2, bn2.weight)
    assert _close(dg2, bn2.weight.grad) and _close(db2, bn2.bias.grad)
    # Shift_gcn.bn's backward with dy = k1*dA + k2*h + k3 formed on the fly
    part, rpart = sr.bn_bwd_reduce(dA, h, True, zu, mean, invstd, 3, r if rs else None,
                                   rs[0] if rs else None, rs[1] if rs else None, dy_coef=k)
    assert part.shape == (B, C, V, 2)
    dg, db, coef = sr.bn_bwd_coef(part.reshape(B, C * V, 2), B * T, mean, invstd, g1)
    assert _close(dg, _loc(bn1.weight.grad, C, V)) and _close(db, _loc(bn1.bias.grad, C, V))
    rcoef = None
    if rs:
        rdg, rdb, rcoef = sr.bn_bwd_coef(rpart, B * T * V, rs[0], rs[1], rbn.weight)
        assert _close(rdg, rbn.weight.grad) and _close(rdb, rbn.bias.grad)
    dzu, dr = sr.bn_bwd_apply(dA, h, True, zu, coef, 3, r if rs else None, rcoef,
                              want_dr=res == "identity", dy_coef=k)
    assert _close(dzu, zu.grad)                               # pre-rotation layout
    if res != "none":
        assert _close(dr, r.grad)


def test_bn_eval_coef_matches_eval_batchnorm():
    C, V, N = 5, 7, 4
    for perm_V, bn, x in ((V, nn.BatchNorm1d(V * C).double(), _t((N, V * C), 21)),
                          (0, nn.BatchNorm2d(C).double(), _t((N, C, 3, V), 22))):
        F = bn.num_features
        with torch.no_grad():
            bn.weight.copy_(_t((F,), 23, 0.4, 1.0))
            bn.bias.copy_(_t((F,), 24, 0.3))
            bn.running_mean.copy_(_t((F,), 25, 0.5))
            bn.running_var.copy_(_t((F,), 26, 0.3, 1.0))
        bn.eval()
        want = bn(x).detach()
        mean, invstd, scale, shift = sr.bn_eval_coef(bn.weight, bn.bias, bn.running_mean,
                                                     bn.running_var, bn.eps, perm_V)
        if perm_V:
            xl = x.view(N, V, C).permute(0, 2, 1).reshape(N, C * V)     # local c*V + v
            got = (xl * scale + shift).view(N, C, V).permute(0, 2, 1).reshape(N, V * C)
            assert _close(mean, _loc(bn.running_mean, C, V), 0.0)
        else:
            got = x * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1)
        assert _close(got, want)
        assert _close(scale, (bn.weight.detach() if not perm_V else _loc(bn.weight.detach(), C, V))
                      * invstd, 0.0)


# --------------------------------------------------------------------------------------
# Shift_gcn input side: the reference's index_select gather and its autograd
# --------------------------------------------------------------------------------------
def _ref_gather(x0, fmask, V, C):
    """shift_gcn.py:125-129 (oracle/model_oracle.py Shift_gcn.forward), back in planes."""
    n, c, t, v = x0.shape
    shift_in = torch.from_numpy(mo.spatial_shift_indices(V, C, +1))
    x = x0.permute(0, 2, 3, 1).contiguous().view(n * t, v * c)
    x = torch.index_select(x, 1, shift_in).view(n * t, v, c)
    x = x * (torch.tanh(fmask) + 1)
    return x.view(n, t, v, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize("C,V", [(5, 7), (9, 4), (3, 1)])
def test_gcn_gather_dx_finish_mask_grad(C, V):
    B, T = 2, 3
    shape = (B, C, T, V)
    x0 = sc.act(shape, 31).double().requires_grad_(True)
    fmask = _t((1, V, C), 32, 0.8).requires_grad_(True)
    dxt = _t(shape, 33)
    xg_t = _ref_gather(x0, fmask, V, C)
    xg_t.backward(dxt)
    m = sr.mask_prep(fmask.detach()).view(V, C)
    assert _close(sr.gcn_gather(x0.detach(), m), xg_t.detach(), 0.0)
    x0d = x0.detach()
    dx, dpart, pp = sr.gcn_dx_finish(dxt, x0d, m)
    assert pp is None and dpart.shape == (B, C, V)
    assert _close(dx, x0.grad)
    assert _close(sr.mask_grad_finalize(dpart, fmask.detach()), fmask.grad)
    prior = _t((1, V, C), 34)
    assert _close(sr.mask_grad_finalize(dpart, fmask.detach(), accumulate=prior),
                  prior + fmask.grad)
    # the additive forms, the masked identity-residual gradient, prev_part and mask_dx
    add1, add2, a2m = _t(shape, 35), _t(shape, 36), sc.act(shape, 37).double()
    S, pmean, pinv = _t(shape, 38), _t((C,), 39, 0.3), _t((C,), 40, 0.4, 1.0)
    base = x0.grad
    masked2 = torch.where(a2m > 0, add2, torch.zeros_like(add2))
    a2p = _t((B, C), 41)
    forms = [
        (dict(add1=add1), base + add1),
        (dict(add2=add2), base + add2),
        (dict(add1=add1, add2=add2), base + add1 + add2),
        (dict(add1=add1, add2=add2, add2_mask=a2m), base + add1 + masked2),
        (dict(add1=add1, add2=a2p, add2_mask=a2m),
         base + add1 + torch.where(a2m > 0, a2p[:, :, None, None].expand(shape),
                                   torch.zeros_like(add2))),
    ]
    for kw, want in forms:
        for mask_dx in (False, True):
            dx, dp, pp = sr.gcn_dx_finish(dxt, x0d, m, prev=(S, pmean, pinv), mask_dx=mask_dx,
                                          **kw)
            assert _close(dx, torch.where(x0d > 0, want, torch.zeros_like(want)) if mask_dx
                          else want)
            assert _close(dp, dpart, 0.0)
            ref_pp, _ = sr.bn_bwd_reduce(want, x0d, True, S, pmean, pinv, 0)
            assert _close(pp, ref_pp)
    # the select: inf behind the mask never reaches dx
    bad = torch.where(a2m > 0, add2, torch.full_like(add2, float("inf")))
    dx, _, _ = sr.gcn_dx_finish(dxt, x0d, m, add1=add1, add2=bad, add2_mask=a2m)
    assert torch.isfinite(dx).all() and _close(dx, forms[3][1], 0.0)


# --------------------------------------------------------------------------------------
# shift-fused restatements against the composed ones
# --------------------------------------------------------------------------------------
def _pos(C, H, variant):
    return sc.positions(C, H, variant)


@pytest.mark.parametrize("stride,H", [(1, 9), (2, 9)])
@pytest.mark.parametrize("rbn", [False, True])
def test_tshift_fwd_pre_and_tail_compose(stride, H, rbn):
    B, C, W = 2, 8, 5
    shape = (B, C, H, W)
    xpos, ypos = _pos(C, H, 0)
    z, r = _t(shape, 41), _t(shape, 42)
    zs, zt = _t((C * W,), 43, 0.4, 1.0), _t((C * W,), 44, 0.3)
    rsc, rsh = (_t((C,), 45, 0.4, 1.0), _t((C,), 46, 0.3)) if rbn else (None, None)
    asc, ash = _t((C,), 47, 0.4, 1.0), _t((C,), 48, 0.3)
    got = sr.tshift_fwd_pre(z, xpos, ypos, stride, zs, zt, r, rsc, rsh, asc, ash)
    h = sr.bn_apply(sr.prerotated(z), zs, zt, 3, r, rsc, rsh, relu=True)
    a = sr.bn_apply(h, asc, ash, 0)
    ye = so.effective_ypos(ypos.numpy(), stride).astype(np.float64)
    want = so.shift_forward(a.numpy(), xpos.numpy().astype(np.float64), ye, stride)
    assert got.shape == (B, C, H // stride, W)
    assert _close(got, torch.from_numpy(want))
    # tail
    inp = _t(shape, 49)
    oshape = (B, C, H // stride, W)
    ro = _t(oshape, 50)
    m = _t((W, C), 51, 0.5, 1.0)
    s = torch.from_numpy(so.shift_forward(inp.numpy(), xpos.numpy().astype(np.float64), ye, stride))
    for rr, rs_, rh_ in ((None, None, None), (ro, None, None), (ro, rsc, rsh)):
        if rr is not None and rbn != (rs_ is not None):
            continue
        out, og = sr.tshift_fwd_tail(inp, xpos, ypos, stride, asc, ash, rr, rs_, rh_, gather_m=m)
        want, wg = sr.bn_apply(s, asc, ash, 0, rr, rs_, rh_, relu=True, gather_m=m)
        assert _close(out, want) and _close(og, wg)
        assert sr.tshift_fwd_tail(inp, xpos, ypos, stride, asc, ash, rr, rs_, rh_)[1] is None


@pytest.mark.parametrize("form", ["y", "premasked", "plane"])
def test_tshift_bwd_bnin_composes(form):
    shape = (3, 8, 9, 5)
    B, C, H, W = shape
    dy, y, s, coef, inp, xpos, ypos = sc.bnin_inputs(shape, 0, plane_dy=form == "plane")
    assert sc.has_all_signs(y) and sc.has_all_signs(inp)
    full = dy[:, :, None, None].expand(shape) if form == "plane" else dy
    if form == "premasked":
        got = sr.tshift_bwd_bnin(torch.where(y > 0, dy, torch.zeros_like(dy)), None, s, coef,
                                 inp, xpos, ypos)
    else:
        got = sr.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos)
    gout, _ = sr.bn_bwd_apply(full, y, True, s, coef, 0)
    xp, yp = xpos.numpy().astype(np.float64), ypos.numpy().astype(np.float64)
    gin, gx, gy = so.shift_backward(gout.numpy(), inp.double().numpy(), xp, yp, 1)
    gin = np.where(inp.numpy() > 0, gin, 0.0)
    assert _close(got[0], torch.from_numpy(gin))
    assert got[1].shape == (B, C, 2)
    assert np.array_equal(got[2].numpy(), gx) and np.array_equal(got[3].numpy(), gy)
    gxb, gyb = so.shift_position_backward(inp.double().numpy(), gout.numpy(), xp, yp, 1)
    assert _close(got[4][:, 1], torch.from_numpy(so.reduce_position_grad(gyb)), 1e-10)
    # the channel with every tap out of range: exact zero sums, gy = 0.0001
    dead = [c for c in range(C) if abs(float(ypos[c])) > H]
    assert dead and all(float(got[4][c, 1]) == 0.0 and float(got[3][c]) == 1e-4 for c in dead)


# --------------------------------------------------------------------------------------
# the shape table: coverage of the launch forms, and the gx / gy seeds
# --------------------------------------------------------------------------------------
def _forms(form, table):
    return {form(T, V) for _, _, T, V in table} - {"refuse"}


def test_table_reaches_every_reachable_launch_form():
    all_ja = {("ja", nt, l) for nt in (256, 512) for l in (8, 16, 24, 32)}
    all_pad = ({("pad", 256, l) for l in (8, 16, 24, 32)} |
               {("pad", 512, l) for l in (8, 12, 16, 20, 24, 32)})
    all_ra = ({("ra", 256, l) for l in (8, 16, 24, 32)} |
              {("ra", 512, l) for l in (8, 12, 16, 20, 24, 32)})
    # BatchNorm plane kernels and gcn_dx_finish (one chooser)
    reach = sc.reachable(sc.bn_form)
    assert _forms(sc.bn_form, sc.TABLE) == reach
    assert "loop" in reach
    assert all_ja - reach == {("ja", 512, 8), ("ja", 512, 16)}        # never launched
    # both routes into the looping kernels: V > 64, and V <= 64 with > 32 per thread
    loops = [(T, V) for _, _, T, V in sc.TABLE if sc.bn_form(T, V) == "loop"]
    assert any(V > 64 for _, V in loops) and any(V <= 64 and T * V <= 8192 for T, V in loops)
    assert any(V <= 64 and T * V > 8192 for T, V in loops)
    # padded forward + fallbacks (sgcn_tshift_fwd_pre / _tail)
    reach = sc.reachable(sc.fwd_form)
    assert _forms(sc.fwd_form, sc.SHIFT_TABLE) == reach
    assert all_pad - reach == {("pad", 512, 8), ("pad", 512, 12), ("pad", 512, 16)}
    assert {f for f in reach if f[0] == "fallback"} == {
        ("fallback", 256, 8), ("fallback", 256, 16), ("fallback", 256, 32), ("fallback", 512, 32)}
    assert _forms(sc.fwd_form, sc.STRIDE2) <= reach
    # stride-1 backward (sgcn_tshift_bwd_bnin)
    reach = sc.reachable(sc.bnin_form)
    assert _forms(sc.bnin_form, sc.SHIFT_TABLE) == reach
    assert all_ra - reach == {("ra", 512, 8), ("ra", 256, 32)}
    # the boundaries the table names
    assert sc.bn_form(80, 25) == ("ja", 256, 8) and sc.bn_form(81, 25) == ("ja", 256, 16)
    assert sc.bn_form(320, 25) == ("ja", 256, 32) and sc.bn_form(325, 25) == "loop"
    assert sc.bn_form(328, 25) == ("ja", 512, 24) and sc.bn_form(240, 33) == "loop"
    assert sc.bn_form(128, 64) == ("ja", 256, 32) and sc.bn_form(129, 64) == ("ja", 512, 24)
    assert sc.bn_form(640, 25) == ("ja", 512, 32) and sc.bn_form(641, 25) == "loop"
    assert sc.bn_form(3, 256) == "loop" and sc.bn_form(3, 257) == "refuse"
    assert sc.bnin_form(163, 25) == ("ra", 256, 24) and sc.bnin_form(164, 25) == ("ra", 512, 12)
    assert sc.fwd_form(300, 33) == ("pad", 512, 20) and sc.bnin_form(300, 33) == ("ra", 512, 20)
    assert sc.fwd_form(598, 25) == ("pad", 512, 32)
    assert sc.fwd_form(599, 25) == ("fallback", 512, 32)
    assert sc.bnin_form(598, 25) == ("ra", 512, 32) and sc.bnin_form(599, 25) == "refuse"
    assert sc.fwd_form(40, 70) == ("fallback", 256, 16)
    assert sc.fwd_form(656, 25) == "refuse"                           # 16,400 floats


def test_ra_fits_agrees_with_the_bnin_chooser():
    """ops.ra_fits (pure Python) accepts exactly the planes sgcn_tshift_bwd_bnin launches."""
    from shiftgcn import ops
    for V in range(1, 80):
        for T in range(1, (sc.K_BWD_LDS_MAX + 300) // V + 2):
            assert ops.ra_fits(T * V, V) == (sc.bnin_form(T, V) != "refuse"), (T, V)
    for _, _, T, V in sc.SHIFT_TABLE:
        assert ops.ra_fits(T * V, V) == (sc.bnin_form(T, V) != "refuse")


def test_every_position_entry_lands_on_a_channel():
    for C in (1, 2, 3, 5, 53):
        seen = set()
        for v in range(sc.n_variants(C)):
            xp, yp = sc.shift_positions(C, 300, v)
            seen |= set(zip(xp, yp))
        assert len(seen) == 8
        ys = [abs(y) for _, y in seen]
        assert any(4 < y < 300 for y in ys) and any(y > 300 for y in ys) and 0.0 in ys
        assert {1.5, -2.25, 0.0} <= {x for x, _ in seen}


@pytest.mark.parametrize("shape",
                         [s for s in sc.SHIFT_TABLE if sc.bnin_form(s[2], s[3]) != "refuse"],
                         ids=lambda s: "x".join(map(str, s)))
def test_bnin_seeds_leave_no_channel_out(shape):
    """The fp64 reference alone leaves no gy channel within GY_REL of a zero plane sum, so
    the GPU test's exact comparison of the finalized gx / gy covers every channel."""
    for variant in range(sc.n_variants(shape[1])):
        for plane in (False, True):
            dy, y, s, coef, inp, xpos, ypos = sc.bnin_inputs(shape, variant, plane_dy=plane)
            _, part, _, _, mean = sr.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos)
            assert not sc.gy_unsafe(part, mean).any(), (variant, plane, mean[:, 1])
