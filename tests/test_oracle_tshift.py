"""Pin the float64 restatements of the temporal-shift entry points (oracle/tshift_ref.py)
without a GPU: against oracle/torch_shift.py and its autograd in double, against
nn.BatchNorm1d / BatchNorm2d and autograd through the whole Shift_gcn.bn -> ReLU ->
Shift_tcn.bn -> shift chain; and check that the shape table of tests/test_gpu_tshift_ref.py
reaches every launch form of sgcn_tshift_fwd / _bwd / _bwd_gbn a plane can reach
(oracle/tshift_cases.py mirrors the launch choosers), that ops.ra_fits accepts exactly the
planes sgcn_tshift_bwd_gbn launches, and that the table's seeds leave no gx / gy channel out
of the GPU test's exact comparison.

Template instances no plane can reach (instantiated, never launched; the enumeration below
asserts each of these sets):

* tshift_fwd_pad_kernel 512 x 8, 512 x 12, 512 x 16: 512 threads are chosen only above 8,192
  floats, and (512 / W) * W <= 512 lanes then hold at least 17 elements each.
* tshift_fwd_kernel (global taps, planes above 16,384 floats) with 8 or 16 outputs per
  thread: at most 4,096 outputs of more than 16,384 inputs needs stride >= 4, or stride 3
  with W >= 2,049; and its single-pass 32 form at stride 1 (one pass is at most 8,192
  outputs).
* tshift_bwd_ra_kernel behind sgcn_tshift_bwd and sgcn_tshift_bwd_gbn without a down conv:
  512 x 8 and 512 x 12. 512 threads are chosen only when 256 x 32 does not cover the plane,
  i.e. above 32 * (256 / W) * W >= 6,656 floats (W = 52), and 12 * (512 / W) * W never
  reaches that many at the same W.
* tshift_bwd_ra_kernel with the down conv's sums (GBD): 512 x 8 as above, and 256 x 32,
  which SGCN_GBD_SPLIT sends to 512 threads (512 x 12 and 512 x 16 are reachable here).
* tshift_bwd_kernel<STRIDE = 2> with 8 or 16 per thread, or 32 in one pass: stride 2 takes
  the global taps only above (H + H / 2) * W = 16,384, i.e. H * W > 10,922 > 8,192.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import shift_oracle as so
from oracle import stream_cases as sc
from oracle import stream_ref as sr
from oracle import torch_shift as ts
from oracle import tshift_cases as tc
from oracle import tshift_ref as tr

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


def _ypos_eff(ypos, stride):
    return torch.from_numpy(so.effective_ypos(ypos.numpy(), stride)).double()


# --------------------------------------------------------------------------------------
# the restatement against torch_shift, autograd and BatchNorm
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("stride,H", [(1, 9), (2, 9), (2, 8), (3, 10)])
def test_forward_matches_torch_shift(stride, H, affine):
    B, C, W = 2, 8, 5                      # C = 8: every entry of the position cycle
    shape = (B, C, H, W)
    inp, xpos, ypos, scale, shift = tc.fwd_inputs(shape, 0, stride)
    if not affine:
        scale = shift = None
    out, stats = tr.tshift_fwd(inp, xpos, ypos, stride, scale, shift)
    pre = inp.double() if not affine else (inp.double() * scale.double().view(1, C, 1, 1)
                                           + shift.double().view(1, C, 1, 1))
    want = ts.shift_forward(pre, xpos.double(), _ypos_eff(ypos, stride), stride)
    assert out.shape == (B, C, H // stride, W) and out.dtype == F64
    assert _close(out, want)
    n = (H // stride) * W
    assert _close(stats[..., 0], want.mean((2, 3)))
    assert _close(stats[..., 1], want.var((2, 3), unbiased=False) * n)
    # a shift with every tap out of range gives 0 whatever the affine's shift[c]
    dead = [c for c in range(C) if abs(float(ypos[c])) > H + 1]
    assert dead and all(float(out[:, c].abs().max()) == 0.0 for c in dead)
    if affine:
        assert all(float(shift[c]) != 0.0 for c in dead)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("stride,H", [(1, 9), (2, 9), (2, 8)])
def test_backward_matches_torch_shift_and_autograd(stride, H, affine):
    B, C, W = 3, 8, 5
    shape = (B, C, H, W)
    k = tc.bwd_inputs(shape, 0, stride)
    gout, inp, xpos, ypos = k["gout"], k["inp"], k["xpos"], k["ypos"]
    scale, shift = (k["scale"], k["shift"]) if affine else (None, None)
    assert sc.has_all_signs(inp)
    # autograd through the differentiable torch restatement of the forward: the input
    # gradient is d/d(pre-affined input), the position sums d/d(xpos, ypos)
    pre = inp.double() if not affine else (inp.double() * scale.double().view(1, C, 1, 1)
                                           + shift.double().view(1, C, 1, 1))
    pre = pre.requires_grad_(True)
    xp = xpos.double().requires_grad_(True)
    yp = _ypos_eff(ypos, stride).requires_grad_(True)
    ts.shift_forward(pre, xp, yp, stride).backward(gout.double())
    for relu in (False, True):
        gin, part, bn_part, gx, gy, mean = tr.tshift_bwd(
            gout, inp, xpos, ypos, stride, scale, shift, relu, k["bn_mean"], k["bn_invstd"])
        want = pre.grad if not relu else torch.where(inp > 0, pre.grad, torch.zeros_like(pre.grad))
        assert _close(gin, want)
        assert _close(gin, ts.shift_backward(gout.double(), pre.detach(), xp.detach(),
                                             yp.detach(), stride)[0]
                      if not relu else want)
        assert part.shape == (B, C, 2)
        assert _close(part[..., 0].sum(0), xp.grad, 1e-10)
        assert _close(part[..., 1].sum(0), yp.grad, 1e-10)
        assert _close(mean, part.mean(0))
        # bn_part: sums of the returned gin written out
        xhat = ((inp.double() - k["bn_mean"].double().view(1, C, 1, 1))
                * k["bn_invstd"].double().view(1, C, 1, 1))
        assert _close(bn_part[..., 0], want.sum((2, 3)))
        assert _close(bn_part[..., 1], (want * xhat).sum((2, 3)))
    # the finalized gradients: the constraint of torch_shift on the same sums
    _, tgx, tgy = ts.shift_backward(gout.double(), pre.detach(), xp.detach(), yp.detach(), stride)
    assert torch.equal(gy, tgy) and torch.equal(gx.abs(), tgx.abs())
    dead = [c for c in range(C) if abs(float(ypos[c])) > H + 1]
    assert dead and all(float(mean[c, 1]) == 0.0 and float(gy[c]) == 1e-4 for c in dead)
    assert tr.tshift_bwd(gout, inp, xpos, ypos, stride)[2] is None


def test_empty_output_plane():
    """H // stride == 0: no output, a zero input gradient, zero partials, gy = 0.0001."""
    shape = tc.EMPTY
    B, C, H, W = shape
    k = tc.bwd_inputs(shape, 0, 2)
    out, stats = tr.tshift_fwd(k["inp"], k["xpos"], k["ypos"], 2)
    assert out.shape == (B, C, 0, W) and stats is None
    gin, part, bn_part, gx, gy, _ = tr.tshift_bwd(k["gout"], k["inp"], k["xpos"], k["ypos"], 2,
                                                  k["scale"], k["shift"], True, k["bn_mean"],
                                                  k["bn_invstd"])
    assert gin.shape == shape and not gin.any() and not part.any() and not bn_part.any()
    assert torch.equal(gy, torch.full((C,), 1e-4, dtype=F64)) and not gx.any()


def test_pos_finalize_branches():
    part = tc.finalize_inputs(33, 5)
    gx, gy, mean = tr.pos_finalize(part)
    assert float(gy[0]) == 1e-4 and float(gx[0]) == 0.0          # dr == 0
    assert float(mean[1, 1]) > 0 and float(gy[1]) == 0.01        # cancels to a small mean
    assert float(gy[2]) == -0.01 and not gx.any()
    assert not sc.gy_unsafe(part.double(), mean).any()


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("C", [5, 9])     # C > V: the rotation wraps
def test_gbn_sums_against_autograd(C, down):
    """Shift_gcn.bn (BatchNorm1d(V*C) over the logical z) [+ the down conv's BatchNorm2d] ->
    ReLU -> Shift_tcn.bn -> shift, differentiated by autograd in double: the six sums of
    tshift_bwd_gbn finalized by bn_bwd_finalize_gbn give both BatchNorms' dgamma / dbeta and
    the coefficients of their input gradients."""
    B, T, V = 3, 6, 7
    shape = (B, C, T, V)
    zu = _t(shape, 11, 2.0, 0.3).requires_grad_(True)
    d = _t(shape, 12, 1.5, -0.2).requires_grad_(True)
    gout = _t(shape, 13)
    xpos, ypos = sc.positions(C, T, 0)
    bn_g = nn.BatchNorm1d(V * C).double()
    bn_d, bn_t = nn.BatchNorm2d(C).double(), nn.BatchNorm2d(C).double()
    with torch.no_grad():
        for i, bn in enumerate((bn_g, bn_d, bn_t)):
            bn.weight.copy_(_t((bn.num_features,), 14 + 2 * i, 0.4, 1.0))
            bn.bias.copy_(_t((bn.num_features,), 15 + 2 * i, 0.3))
    z = sr.logical(zu)
    zf = z.permute(0, 2, 3, 1).reshape(B * T, V * C)            # feature v*C + c
    a = bn_g(zf).view(B, T, V, C).permute(0, 3, 1, 2)
    if down:
        a = a + bn_d(d)
    h = torch.relu(a)
    h.retain_grad()
    out = ts.shift_forward(bn_t(h), xpos.double(), ypos.double(), 1)
    out.backward(gout)

    hd = h.detach()
    assert (hd == 0).any() and (hd > 0).any()
    n = T * V
    g_loc = _loc(bn_g.weight.detach(), C, V)
    zm, zi, _, _ = sr.bn_train_stats(sr.moments(zu, 3).reshape(B, C * V, 2), T, g_loc,
                                     _loc(bn_g.bias.detach(), C, V), bn_g.eps)
    tm, ti, tsc, tsh = sr.bn_train_stats(sr.moments(hd, 0), n, bn_t.weight, bn_t.bias, bn_t.eps)
    dm, di, _, _ = sr.bn_train_stats(sr.moments(d, 0), n, bn_d.weight, bn_d.bias, bn_d.eps)
    res = tr.tshift_bwd_gbn(gout, hd, xpos, ypos, tsc, tsh, tm, ti, zu, zm, zi,
                            *((d, dm, di) if down else ()))
    gin, bn_part, z_part, d_part = res[0], res[2], res[6], res[7]
    assert z_part.shape == (6, B, C, V) and (d_part is None) == (not down)
    # the same call without the extra sums
    ref = tr.tshift_bwd(gout, hd, xpos, ypos, 1, tsc, tsh, False, tm, ti)
    assert all(torch.equal(u, v) for u, v in zip(res[:6], ref))
    # Shift_tcn.bn
    dg, db, kt = sr.bn_bwd_coef(bn_part, B * n, tm, ti, bn_t.weight)
    assert _close(dg, bn_t.weight.grad) and _close(db, bn_t.bias.grad)
    k4 = kt.view(3, 1, C, 1, 1)
    assert _close(k4[0] * gin + k4[1] * hd + k4[2], h.grad)
    # the six sums written out with a gather, kind by kind
    act = hd > 0
    idx = (torch.arange(V)[None, :] - torch.arange(C)[:, None]) % V
    zl = zu.detach().gather(3, idx.view(1, C, 1, V).expand(shape))
    zh = (zl - zm.view(1, C, 1, V)) * zi.view(1, C, 1, V)
    hc = hd - tm.view(1, C, 1, 1)
    kinds = (gin, hc, torch.ones_like(gin), gin * zh, hc * zh, zh)
    for j, kind in enumerate(kinds):
        assert _close(z_part[j], (kind * act).sum(2)), j
    # Shift_gcn.bn
    dg, db, coef = tr.bn_bwd_finalize_gbn(z_part, B * T, kt, tm, zm, zi, g_loc)
    assert _close(dg, _loc(bn_g.weight.grad, C, V), 1e-10)
    assert _close(db, _loc(bn_g.bias.grad, C, V), 1e-10)
    g = torch.where(act, h.grad, torch.zeros_like(h.grad))
    kz = coef.view(3, 1, C, 1, V)
    assert _close(sr.prerotated(kz[0] * g + kz[1] * zl + kz[2]), zu.grad, 1e-10)
    if down:
        dh = (d.detach() - dm.view(1, C, 1, 1)) * di.view(1, C, 1, 1)
        for j, kind in enumerate((gin, hc, torch.ones_like(gin), gin * dh, hc * dh, dh)):
            assert _close(d_part[j], (kind * act).sum((2, 3))), j
        dg, db, coef = tr.bn_bwd_finalize_gbn(d_part, B * n, kt, tm, dm, di, bn_d.weight)
        assert _close(dg, bn_d.weight.grad, 1e-10) and _close(db, bn_d.bias.grad, 1e-10)
        kd = coef.view(3, 1, C, 1, 1)
        assert _close(kd[0] * g + kd[1] * d.detach() + kd[2], d.grad, 1e-10)


# --------------------------------------------------------------------------------------
# the shape table: coverage of the launch forms, chooser consistency, the gx / gy seeds
# --------------------------------------------------------------------------------------
def _forms(form, table):
    return {form(s[2], s[3]) for s in table} - {"refuse"}


def test_table_reaches_every_reachable_launch_form():
    all_pad = ({("pad", 256, l) for l in (8, 16, 24, 32)} |
               {("pad", 512, l) for l in (8, 12, 16, 20, 24, 32)})
    all_lds = {("lds", 256, 8), ("lds", 256, 16), ("lds", 256, 32), ("lds", 512, 32)}
    all_glob = {("global", e, lp) for e in (8, 16, 32) for lp in (False, True)
                if lp <= (e == 32)}              # 8 / 16 per thread cover their plane in one pass
    all_ra = ({("ra", 256, l) for l in (8, 16, 24, 32)} |
              {("ra", 512, l) for l in (8, 12, 16, 20, 24, 32)})
    all_s2 = {("s2", l, ja) for l in (8, 16, 32) for ja in (False, True)}
    # sgcn_tshift_fwd
    dead_pad = {("pad", 512, 8), ("pad", 512, 12), ("pad", 512, 16)}
    for stride, dead_glob in ((1, {("global", 8, False), ("global", 16, False),
                                   ("global", 32, False)}),
                              (2, {("global", 8, False), ("global", 16, False)})):
        reach = tc.reachable(lambda H, W: tc.fwd_form(H, W, stride))
        assert _forms(lambda H, W: tc.fwd_form(H, W, stride), tc.TABLE) == reach, stride
        assert (all_pad | all_lds | all_glob) - reach == dead_pad | dead_glob, stride
        assert ("empty" in reach) == (stride == 2)
    assert tc.fwd_form(*tc.EMPTY[2:], 2) == "empty"
    assert all(tc.fwd_form(s[2], s[3], st) != "empty" for s, st in tc.FWD_ONLY)
    # sgcn_tshift_bwd
    reach = tc.reachable(lambda H, W: tc.bwd_form(H, W, 1))
    assert _forms(lambda H, W: tc.bwd_form(H, W, 1), tc.TABLE) == reach
    assert all_ra - reach == {("ra", 512, 8), ("ra", 512, 12)}
    assert {f[2:] for f in reach if f[0] == "global"} == {f[1:] for f in all_glob}
    reach = tc.reachable(lambda H, W: tc.bwd_form(H, W, 2))
    assert _forms(lambda H, W: tc.bwd_form(H, W, 2), tc.TABLE) == reach
    assert {f for f in reach if f[0] == "s2"} == all_s2
    assert {f[2:] for f in reach if f[0] == "global"} == {(32, True)}
    # sgcn_tshift_bwd_gbn
    for down, dead in ((False, {(512, 8), (512, 12)}), (True, {(512, 8), (256, 32)})):
        reach = tc.reachable(lambda H, W: tc.gbn_form(H, W, down))
        assert _forms(lambda H, W: tc.gbn_form(H, W, down), tc.GBN_SHAPES) == reach, down
        assert {f[1:3] for f in all_ra} - {f[1:3] for f in reach} == dead, down
        assert all(f[3] == down for f in reach)
    assert any(tc.gbn_form(s[2], s[3], False) == "refuse" for s in tc.GBN_SHAPES)
    # the boundaries the table names
    assert tc.fwd_form(655, 25, 1) == ("lds", 512, 32)
    assert tc.fwd_form(656, 25, 1) == ("global", 32, True)
    assert tc.fwd_form(497, 33, 2) == ("global", 32, False)
    assert tc.bwd_form(85, 65, 2) == ("s2", 32, False)
    assert tc.bwd_form(301, 25, 2) == ("s2", 32, True)
    assert tc.bwd_form(656, 25, 2) == ("global", 2, 32, True)
    assert tc.bwd_form(641, 25, 1) == ("global", 1, 32, True)
    assert tc.bwd_form(300, 25, 1) == ("ra", 256, 32) and tc.bwd_form(300, 33, 1) == ("ra", 512, 20)
    assert tc.gbn_form(169, 33, True) == ("ra", 512, 12, True)
    assert tc.gbn_form(169, 33, False) == ("ra", 256, 32, False)
    assert tc.gbn_form(300, 25, True) == ("ra", 512, 16, True)
    # 256 threads at 6 * W > 256: the merge of the per-joint sums takes a second round
    # (W = 64: sums 4 and 5 entirely; one round left them unwritten)
    assert tc.gbn_form(128, 64, False) == ("ra", 256, 32, False)
    assert tc.gbn_form(128, 64, True) == ("ra", 512, 16, True)
    assert any(6 * s[3] > 256 and tc.gbn_form(s[2], s[3], False)[1] == 256 for s in tc.GBN_SHAPES)


def test_stride1_backward_agrees_with_the_stream_mirrors():
    """sgcn_tshift_bwd's padded forward and joint-aligned backward use the choosers of the
    shift-fused entry points: where both mirrors name a padded / joint-aligned form the
    per-thread counts agree, and the plain backward launches every plane bnin does."""
    for W in range(1, 80):
        for H in range(1, (sc.K_BWD_LDS_MAX + 300) // W + 2):
            f = sc.fwd_form(H, W)
            if f != "refuse" and f[0] == "pad":
                assert tc.fwd_form(H, W, 1) == f, (H, W)
            if sc.bnin_form(H, W) != "refuse":
                assert tc.bwd_form(H, W, 1)[0] == "ra", (H, W)


def test_ra_fits_agrees_with_the_gbn_chooser():
    """ops.ra_fits (pure Python) accepts exactly the planes sgcn_tshift_bwd_gbn launches,
    without and with the down conv's sums."""
    from shiftgcn import ops
    for W in range(1, 131):
        for H in range(1, (sc.K_BWD_LDS_MAX + 2 * 256) // W + 2):
            fits = ops.ra_fits(H * W, W)
            assert fits == (tc.gbn_form(H, W, False) != "refuse"), (H, W)
            assert fits == (tc.gbn_form(H, W, True) != "refuse"), (H, W)


def test_per_channel_inputs_are_distinct():
    for shape in ((1, 2, 7, 25), (1, 3, 7, 25)):
        k = tc.bwd_inputs(shape, 0, 1)
        for name in ("scale", "shift", "bn_mean", "bn_invstd", "d_mean", "d_invstd"):
            assert k[name].unique().numel() == shape[1], name
        zm = k["z_mean"].view(shape[1], shape[3])
        assert not torch.equal(zm[0], zm[1])
        _, _, _, scale, shift = tc.fwd_inputs(shape, 0, 1)
        assert scale.unique().numel() == shape[1] and shift.unique().numel() == shape[1]
    for shape, _ in tc.BWD_CASES:
        assert shape[0] * shape[1] >= 2 and shape[1] >= 2


@pytest.mark.parametrize("case", tc.BWD_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-s{c[1]}")
def test_seeds_leave_no_channel_out(case):
    """The fp64 reference alone leaves no gy channel within GY_REL of a zero plane sum, with
    and without the affine taps, so the GPU test's exact comparison of the finalized gx / gy
    covers every channel of every case (its cap of one channel left out is never used)."""
    shape, stride = case
    for variant in range(tc.n_variants(shape[1])):
        k = tc.bwd_inputs(shape, variant, stride)
        assert sc.has_all_signs(k["inp"]) or k["inp"].numel() < 8
        for aff in (False, True):
            res = tr.tshift_bwd(k["gout"], k["inp"], k["xpos"], k["ypos"], stride,
                                k["scale"] if aff else None, k["shift"] if aff else None)
            assert not sc.gy_unsafe(res[1], res[5]).any(), (variant, aff, res[5][:, 1])


@pytest.mark.parametrize("B", [1, 31, 32, 33, 70])
def test_finalize_seeds_leave_no_channel_out(B):
    for C in (1, 3, 4, 5, 67):
        part = tc.finalize_inputs(B, C)
        gx, gy, mean = tr.pos_finalize(part)
        assert not sc.gy_unsafe(part.double(), mean).any(), (B, C)
        assert float(gy[0]) == 1e-4
        if C > 2:
            assert float(mean[1, 1]) >= 0.5 and float(gy[1]) == 0.01 and float(gy[2]) == -0.01
