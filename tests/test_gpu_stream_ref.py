"""The streaming kernels against their float64 restatements (oracle/stream_ref.py) at every
launch form: the BatchNorm plane kernels, sgcn_gcn_gather / sgcn_gcn_dx_finish, the mask
kernels, sgcn_bn_eval_coef and the shift-fused sgcn_tshift_fwd_pre / _tail / _bwd_bnin.

The shapes (oracle/stream_cases.py) are the smallest that reach each (threads, per-thread)
instantiation, each fallback and each threshold between them; tests/test_oracle_stream.py
checks that coverage, and pins the restatements, without a GPU.

Bars (max |got - ref| <= bar * max |ref| over the output):
  E6  = 1e-6  element-wise outputs of a handful of fp32 operations (test_gpu_zu.py's bar);
  E5  = 1e-5  outputs that pass through the four-tap blend or k1*dy + k2*s + k3 (DESIGN's
              kernel bar, the shift's north-star bound), which can cancel;
  SUM = 1e-5  plane and joint sums (moments, part, rpart, dmask_part, prev_part, position
              partials), each component of the output taken as its own vector.
The finalized gx / gy of bnin are compared exactly (see _check_pos).

Measured on an MI355X (worst case over the table): element-wise outputs 1.1e-7 (E6) and
1.7e-7 (E5); sums 8.6e-7 (moments), 1.2e-6 (part), 3.9e-7 (prev_part), 2.1e-7 (dmask_part),
3.2e-6 (position partials, at (1, 2, 301, 33)): SUM holds unwidened up to the 16,000-term
planes, so no fp32-torch allowance was needed.
"""
import pytest
import torch
import torch.nn as nn

from oracle import stream_cases as sc
from oracle import stream_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
E6, E5, SUM = 1e-6, 1e-5, 1e-5


def _id(s):
    return "x".join(map(str, s))


def _t(shape, seed, scale=1.0, offset=0.0):
    return sc.t(shape, seed, scale, offset).to(DEV)


def _act(shape, seed):
    v = sc.act(shape, seed).to(DEV)
    assert sc.has_all_signs(v)
    return v


def _check(got, ref, bar, what):
    """max |got - ref| <= bar * max |ref|; the figure is printed before it is asserted."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err, mx = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: err {err:.3e} max|ref| {mx:.3e} rel {err / (mx + 1e-300):.2e} bar {bar:.0e}")
    assert err <= bar * mx, (what, err, mx, bar)


def _check_sums(got, ref, what):
    """a (..., k) stack of k kinds of sums: each kind against its own max |ref|"""
    got = got.view(ref.shape)
    for j in range(ref.shape[-1]):
        _check(got[..., j], ref[..., j], SUM, f"{what}[{j}]")


def _stats(F, seed):
    from shiftgcn import ops
    st = ops.BnStats(F, DEV)
    st.mean.copy_(_t((F,), seed, 0.3))
    st.invstd.copy_(_t((F,), seed + 1, 0.4, 1.0))
    st.scale.copy_(_t((F,), seed + 2, 0.5, 1.0))
    st.shift.copy_(_t((F,), seed + 3, 0.2))
    return st


def _expand(p, shape):
    return p[:, :, None, None].expand(*shape).contiguous()


# --------------------------------------------------------------------------------------
# BatchNorm plane kernels
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.TABLE, ids=_id)
def test_moments(shape):
    from shiftgcn import ops
    x = _t(shape, 1, 2.0, 0.3)
    for pj in (0, 3):
        _check_sums(ops.moments(x, pj), sr.moments(x, pj), f"moments pj{pj}")


@pytest.mark.parametrize("shape", sc.TABLE, ids=_id)
def test_bn_apply(shape):
    from shiftgcn import ops
    B, C, T, V = shape
    x, r, m = _t(shape, 2, 2.0, 0.3), _t(shape, 3), _t((V, C), 4, 0.5, 1.0)
    rst = _stats(C, 5)
    for pj in (0, 3):
        st = _stats(C * V if pj else C, 9 + pj)
        for res in (0, 1, 2):
            rr = r if res else None
            rs = rst if res == 2 else None
            rsc, rsh = (rst.scale, rst.shift) if res == 2 else (None, None)
            for relu in ((True, False) if pj == 0 else (True,)):
                tag = f"bn_apply pj{pj} res{res} relu{int(relu)}"
                ref, ref_s = sr.bn_apply(x, st.scale, st.shift, pj, rr, rsc, rsh, relu=relu,
                                         out_stats=True)
                y = ops.bn_apply(x, st, pj, r=rr, rst=rs, relu=relu)
                _check(y, ref, E6, tag)
                y, ys = ops.bn_apply(x, st, pj, r=rr, rst=rs, relu=relu, out_stats=True)
                _check(y, ref, E6, tag + " (+stats)")
                _check_sums(ys, ref_s, tag + " stats")
                if pj == 0:
                    y, yg = ops.bn_apply(x, st, pj, r=rr, rst=rs, relu=relu, gather_m=m)
                    _check(y, ref, E6, tag + " (+gather)")
                    _check(yg, sr.gcn_gather(ref, m), E6, tag + " gathered")


@pytest.mark.parametrize("shape", sc.TABLE, ids=_id)
def test_bn_bwd_reduce_apply(shape):
    from shiftgcn import ops
    B, C, T, V = shape
    dy, y, x, r = _t(shape, 11), _act(shape, 12), _t(shape, 13, 2.0, 0.3), _t(shape, 14)
    dyp, dyc, rst = _t((B, C), 15), _t((3, C), 16, 0.5, 0.25), _stats(C, 17)
    rcoef = _t((3, C), 21, 0.5, 0.25)
    pre = torch.where(y > 0, dy, torch.zeros_like(dy))
    bad = torch.where(y > 0, dy, torch.full_like(dy, float("inf")))
    for pj in (0, 3):
        F = C * V if pj else C
        st, coef = _stats(F, 22 + pj), _t((3, F), 26 + pj, 0.5, 0.25)
        for mode in (("relu", "pre") if pj == 0 else ("relu",)):
            relu = mode == "relu"
            yy = y if relu else None
            for rb in (False, True):
                ra = dict(r=r, rst=rst) if rb else {}
                rr = dict(r=r, rmean=rst.mean, rinvstd=rst.invstd) if rb else {}
                for dc in ((None, dyc) if relu else (None,)):
                    for plane in (False, True):
                        d = dyp if plane else (dy if relu else pre)
                        tag = (f"bn_bwd_reduce pj{pj} {mode} rb{int(rb)} "
                               f"dc{int(dc is not None)} plane{int(plane)}")
                        part, rpart = ops.bn_bwd_reduce(d, yy, relu, x, st, pj, dy_coef=dc, **ra)
                        rp, rrp = sr.bn_bwd_reduce(d, yy, relu, x, st.mean, st.invstd, pj,
                                                   dy_coef=dc, **rr)
                        _check_sums(part, rp, tag + " part")
                        if rb:
                            _check_sums(rpart, rrp, tag + " rpart")
                        else:
                            assert rpart is None
            for res in (0, 1, 2):
                for dc in ((None, dyc) if relu else (None,)):
                    d = dy if relu else pre
                    bar = E5 if dc is not None else E6
                    tag = f"bn_bwd_apply pj{pj} {mode} res{res} dc{int(dc is not None)}"
                    dr = torch.empty_like(x) if res else None
                    dx = ops.bn_bwd_apply(d, yy, relu, x, coef, pj, r=r if res == 2 else None,
                                          rcoef=rcoef if res == 2 else None, dr=dr, dy_coef=dc)
                    rdx, rdr = sr.bn_bwd_apply(d, yy, relu, x, coef, pj,
                                               r=r if res == 2 else None,
                                               rcoef=rcoef if res == 2 else None,
                                               want_dr=res == 1, dy_coef=dc)
                    _check(dx, rdx, bar, tag + " dx")
                    if res:
                        _check(dr, rdr, bar, tag + " dr")
        # the ReLU predicate is a select: inf behind the mask changes nothing
        for dc in (None, dyc):
            p0, q0 = ops.bn_bwd_reduce(dy, y, True, x, st, pj, r=r, rst=rst, dy_coef=dc)
            p1, q1 = ops.bn_bwd_reduce(bad, y, True, x, st, pj, r=r, rst=rst, dy_coef=dc)
            assert torch.isfinite(p1).all() and torch.equal(p0, p1) and torch.equal(q0, q1)
            d0, d1 = torch.empty_like(x), torch.empty_like(x)
            x0 = ops.bn_bwd_apply(dy, y, True, x, coef, pj, dr=d0, dy_coef=dc)
            x1 = ops.bn_bwd_apply(bad, y, True, x, coef, pj, dr=d1, dy_coef=dc)
            assert torch.isfinite(x1).all() and torch.equal(x0, x1) and torch.equal(d0, d1)
            rdx, rdr = sr.bn_bwd_apply(bad, y, True, x, coef, pj, want_dr=True, dy_coef=dc)
            _check(x1, rdx, E5 if dc is not None else E6, f"bn_bwd_apply pj{pj} inf dx")
            _check(d1, rdr, E5 if dc is not None else E6, f"bn_bwd_apply pj{pj} inf dr")


def test_bn_eval_coef():
    from shiftgcn import ops
    C, V = 53, 25
    for perm_V, bn in ((V, nn.BatchNorm1d(V * C)), (0, nn.BatchNorm2d(C)), (1, nn.BatchNorm2d(C))):
        bn = bn.to(DEV)
        F = bn.num_features
        with torch.no_grad():
            bn.weight.copy_(_t((F,), 31, 0.4, 1.0))
            bn.bias.copy_(_t((F,), 32, 0.3))
            bn.running_mean.copy_(_t((F,), 33, 0.5))
            bn.running_var.copy_(_t((F,), 34, 0.3, 1.0))
        st = ops._bn_eval_coef(bn, F, perm_V)
        ref = sr.bn_eval_coef(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, perm_V)
        for got, want, n in zip((st.mean, st.invstd, st.scale, st.shift), ref,
                                ("mean", "invstd", "scale", "shift")):
            _check(got, want, E6, f"bn_eval_coef perm_V{perm_V} {n}")


# --------------------------------------------------------------------------------------
# Shift_gcn input side and the mask kernels
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.TABLE, ids=_id)
def test_gcn_gather(shape):
    from shiftgcn import ops
    B, C, T, V = shape
    x0, m = _act(shape, 41), _t((V, C), 42, 0.5, 1.0)
    _check(ops.gcn_gather(x0, m), sr.gcn_gather(x0, m), E6, "gcn_gather")


@pytest.mark.parametrize("shape", sc.TABLE, ids=_id)
def test_gcn_dx_finish(shape):
    from shiftgcn import ops
    B, C, T, V = shape
    dxt, x0, m = _t(shape, 43), _act(shape, 44), _t((V, C), 45, 0.5, 1.0)
    add1, add2, a2m, a2p = _t(shape, 46), _t(shape, 47), _act(shape, 48), _t((B, C), 49)
    S, pst = _t(shape, 50), _stats(C, 51)
    forms = {
        "none": {}, "add1": dict(add1=add1), "add2": dict(add2=add2),
        "add1+add2": dict(add1=add1, add2=add2),
        "identity": dict(add1=add1, add2=add2, add2_mask=a2m),
        "identity_plane": dict(add1=add1, add2=a2p, add2_mask=a2m),
    }
    for name, kw in forms.items():
        for prev in (False, True):
            for mask_dx in (False, True):
                tag = f"gcn_dx_finish {name} prev{int(prev)} mdx{int(mask_dx)}"
                got = ops.gcn_dx_finish(dxt, x0, m, prev=(S, pst) if prev else None,
                                        mask_dx=mask_dx, **kw)
                ref = sr.gcn_dx_finish(dxt, x0, m, prev=(S, pst.mean, pst.invstd) if prev else None,
                                       mask_dx=mask_dx, **kw)
                assert len(got) == (3 if prev else 2)
                _check(got[0], ref[0], E6, tag + " dx")
                _check(got[1], ref[1], SUM, tag + " dmask_part")
                if prev:
                    _check_sums(got[2], ref[2], tag + " prev_part")
    # selects: inf in add2 behind add2_mask, inf in add1 behind x0 with mask_dx
    bad2 = torch.where(a2m > 0, add2, torch.full_like(add2, float("inf")))
    a = ops.gcn_dx_finish(dxt, x0, m, add1=add1, add2=add2, add2_mask=a2m, prev=(S, pst))
    b = ops.gcn_dx_finish(dxt, x0, m, add1=add1, add2=bad2, add2_mask=a2m, prev=(S, pst))
    assert all(torch.isfinite(v).all() for v in b) and all(torch.equal(u, v) for u, v in zip(a, b))
    ref = sr.gcn_dx_finish(dxt, x0, m, add1=add1, add2=bad2, add2_mask=a2m)
    _check(b[0], ref[0], E6, "gcn_dx_finish inf add2 dx")
    bad1 = torch.where(x0 > 0, add1, torch.full_like(add1, float("inf")))
    a = ops.gcn_dx_finish(dxt, x0, m, add1=add1, prev=(S, pst), mask_dx=True)
    b = ops.gcn_dx_finish(dxt, x0, m, add1=bad1, prev=(S, pst), mask_dx=True)
    assert all(torch.isfinite(v).all() for v in b) and all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("shape", sc.FORM_SHAPES + [(1, 53, 3, 25)], ids=_id)
def test_mask_prep_and_grad_finalize(shape):
    from shiftgcn import ops
    _, C, _, V = shape
    assert (V * C) % 256 != 0
    mask = _t((1, V, C), 52, 0.8)
    _check(ops.mask_prep(mask), sr.mask_prep(mask), E6, "mask_prep")
    for Bp in (1, 5):
        part = _t((Bp, C, V), 53 + Bp)
        ref = sr.mask_grad_finalize(part, mask)
        _check(ops.mask_grad_finalize(part.reshape(-1), mask, Bp, C, V), ref, E6,
               f"mask_grad_finalize B{Bp}")
        prior = _t((1, V, C), 59)
        out = prior.clone()
        got = ops.mask_grad_finalize(part.reshape(-1), mask, Bp, C, V, out=out, accumulate=True)
        assert got is out
        _check(out, sr.mask_grad_finalize(part, mask, accumulate=prior), E6,
               f"mask_grad_finalize B{Bp} accumulate")
        out = prior.clone()
        ops.mask_grad_finalize(part.reshape(-1), mask, Bp, C, V, out=out)
        _check(out, ref, E6, f"mask_grad_finalize B{Bp} overwrite")


# --------------------------------------------------------------------------------------
# shift-fused kernels
# --------------------------------------------------------------------------------------
def _pos(C, H, variant):
    xp, yp = sc.positions(C, H, variant)
    return xp.to(DEV), yp.to(DEV)


FWD_CASES = [(s, 1) for s in sc.SHIFT_TABLE] + [(s, 2) for s in sc.STRIDE2]


def _fwd_id(c):
    return _id(c[0]) + f"-s{c[1]}"


@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_tshift_fwd_pre(case):
    from shiftgcn import ops
    shape, stride = case
    B, C, H, W = shape
    assert sc.fwd_form(H, W) != "refuse"
    z, r = _t(shape, 61, 1.0, 0.2), _t(shape, 62)
    zst, rst, ast = _stats(C * W, 63), _stats(C, 67), _stats(C, 71)
    for variant in range(sc.n_variants(C)):
        xpos, ypos = _pos(C, H, variant)
        for rs in (None, rst):
            got = ops.tshift_fwd_pre(z, xpos, ypos, stride, zst, r, rs, ast)
            ref = sr.tshift_fwd_pre(z, xpos, ypos, stride, zst.scale, zst.shift, r,
                                    rs.scale if rs else None, rs.shift if rs else None,
                                    ast.scale, ast.shift)
            assert got.shape == (B, C, H // stride, W)
            _check(got, ref, E5, f"tshift_fwd_pre v{variant} rbn{int(rs is not None)}")


@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_tshift_fwd_tail(case):
    from shiftgcn import ops
    shape, stride = case
    B, C, H, W = shape
    oshape = (B, C, H // stride, W)
    inp, r, m = _t(shape, 75), _t(oshape, 76), _t((W, C), 77, 0.5, 1.0)
    st, rst = _stats(C, 78), _stats(C, 82)
    for variant in range(sc.n_variants(C)):
        xpos, ypos = _pos(C, H, variant)
        for rr, rs in ((None, None), (r, None), (r, rst)):
            ref, ref_g = sr.tshift_fwd_tail(inp, xpos, ypos, stride, st.scale, st.shift, rr,
                                            rs.scale if rs else None, rs.shift if rs else None,
                                            gather_m=m)
            tag = f"tshift_fwd_tail v{variant} res{int(rr is not None) + int(rs is not None)}"
            out, og = ops.tshift_fwd_tail(inp, xpos, ypos, stride, st, r=rr, rst=rs)
            assert og is None and out.shape == oshape
            _check(out, ref, E5, tag)
            out, og = ops.tshift_fwd_tail(inp, xpos, ypos, stride, st, r=rr, rst=rs, gather_m=m)
            _check(out, ref, E5, tag + " (+gather)")
            _check(og, ref_g, E5, tag + " gathered")


def _check_pos(pp, ref_part, ref_gx, ref_gy, ref_mean, B, C, tag):
    """The per-plane position partials under SUM; the finalized gx / gy (sign-like: +-0.01
    after applyShiftConstraint, 0.0001 for an exactly zero sum) exactly equal to the
    constraint applied to the fp64 batch mean, on every channel whose |fp64 mean| exceeds
    GY_REL x mean |per-plane sum| or is exactly zero (every tap out of range: exact zeros in
    any precision); at most one channel per case may be left out (DESIGN row a6; the seeds
    leave none out, tests/test_oracle_stream.py)."""
    _check_sums(pp.ws[:2 * B * C], ref_part, tag + " pos_part")
    gx = torch.empty((C,), device=DEV)
    gy = torch.empty((C,), device=DEV)
    pp.finalize(gx, gy)
    skip = sc.gy_unsafe(ref_part, ref_mean)
    assert int(skip.sum()) <= 1, (tag, skip)
    keep = ~skip
    assert torch.equal(gy[keep], ref_gy.float()[keep]), (tag, gy, ref_gy)
    assert torch.equal(gx[keep], ref_gx.float()[keep]), (tag, gx, ref_gx)


@pytest.mark.parametrize("shape", sc.SHIFT_TABLE, ids=_id)
def test_tshift_bwd_bnin(shape):
    from shiftgcn import ops
    B, C, H, W = shape
    if sc.bnin_form(H, W) == "refuse":
        # not launched: the plane does not fit the joint-aligned LDS backward
        assert not ops.ra_fits(H * W, W)
        dy, y, s, coef, inp, xpos, ypos = (v.to(DEV) for v in sc.bnin_inputs(shape, 0))
        with pytest.raises(ValueError, match="invalid argument"):
            ops.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos)
        return
    assert ops.ra_fits(H * W, W)
    for variant in range(sc.n_variants(C)):
        for plane in (False, True):
            dy, y, s, coef, inp, xpos, ypos = (
                v.to(DEV) for v in sc.bnin_inputs(shape, variant, plane_dy=plane))
            assert sc.has_all_signs(y) and sc.has_all_signs(inp)
            ref = sr.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos)
            tag = f"tshift_bwd_bnin v{variant} plane{int(plane)}"
            gin, pp, _ = ops.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos, defer_pos=True)
            _check(gin, ref[0], E5, tag + " gin")
            _check_pos(pp, ref[1], ref[2], ref[3], ref[4], B, C, tag)
            if plane:
                continue
            # dy already masked (y = None): the same gradient
            pre = torch.where(y > 0, dy, torch.zeros_like(dy))
            gin, pp, _ = ops.tshift_bwd_bnin(pre, None, s, coef, inp, xpos, ypos, defer_pos=True)
            _check(gin, ref[0], E5, tag + " premasked gin")
            _check_pos(pp, ref[1], ref[2], ref[3], ref[4], B, C, tag + " premasked")
            # the finalize inside the call
            gin, gx, gy = ops.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos)
            keep = ~sc.gy_unsafe(ref[1], ref[4])
            assert torch.equal(gy[keep], ref[3].float()[keep])
            assert torch.equal(gx[keep], ref[2].float()[keep])
            # the predicate on y is a select
            bad = torch.where(y > 0, dy, torch.full_like(dy, float("inf")))
            g2, p2, _ = ops.tshift_bwd_bnin(bad, y, s, coef, inp, xpos, ypos, defer_pos=True)
            assert torch.isfinite(g2).all() and torch.isfinite(p2.ws).all()
            _check(g2, ref[0], E5, tag + " inf gin")
            _check_sums(p2.ws[:2 * B * C], ref[1], tag + " inf pos_part")


# --------------------------------------------------------------------------------------
# refusals
# --------------------------------------------------------------------------------------
def test_refusals():
    from shiftgcn import ops
    shape = (1, 2, 3, 257)
    assert sc.bn_form(3, 257) == "refuse"
    x, y = _t(shape, 91), _act(shape, 92)
    st, stj, m = _stats(2, 93), _stats(2 * 257, 97), _t((257, 2), 98, 0.5, 1.0)
    coef = _t((3, 2), 99)
    calls = [
        lambda: ops.moments(x, 0), lambda: ops.moments(x, 3),
        lambda: ops.bn_apply(x, st, 0), lambda: ops.bn_apply(x, stj, 3, relu=True),
        lambda: ops.bn_bwd_reduce(x, y, True, x, st, 0),
        lambda: ops.bn_bwd_apply(x, y, True, x, coef, 0),
        lambda: ops.gcn_gather(x, m), lambda: ops.gcn_dx_finish(x, y, m),
    ]
    for call in calls:
        with pytest.raises(ValueError, match="invalid argument"):
            call()
    # pre / tail: LDS-staged planes only (H * W <= 16,384)
    shape = (1, 2, 656, 25)
    assert sc.fwd_form(656, 25) == "refuse" and sc.fwd_form(655, 25) != "refuse"
    z, r = _t(shape, 101), _t(shape, 102)
    xpos, ypos = _pos(2, 656, 0)
    with pytest.raises(ValueError, match="invalid argument"):
        ops.tshift_fwd_pre(z, xpos, ypos, 1, _stats(50, 103), r, None, _stats(2, 107))
    with pytest.raises(ValueError, match="invalid argument"):
        ops.tshift_fwd_tail(z, xpos, ypos, 1, _stats(2, 111))
