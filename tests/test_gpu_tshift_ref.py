"""The temporal-shift kernels the training step runs (sgcn_tshift_fwd, sgcn_tshift_bwd,
sgcn_tshift_bwd_gbn, sgcn_tshift_pos_finalize and the float64 entry points) against their
float64 restatements (oracle/tshift_ref.py) at every launch form and with every fused option.

The shapes (oracle/tshift_cases.py) are the smallest that reach each (kernel, threads,
per-thread) instantiation and each threshold between them, at stride 1 and 2;
tests/test_oracle_tshift.py checks that coverage, and pins the restatements, without a GPU.
Every case runs over the position variants that put on some channel a shift inside the LDS
padding, one past it (|floor(y)| >= 4, |x| >= 1: the range-checked loops) and one with every
tap out of range.

Every input is a slice of NaN storage; every tensor an entry point allocates and writes
(outputs, partial sums, workspaces) is handed out at its exact extent between two margins of
a sentinel bit pattern, which must survive the call.

Bars (max |got - ref| <= bar * max |ref| over the output; test_gpu_stream_ref's):
  E5  = 1e-5  outputs and input gradients (the four-tap blend of affine taps);
  SUM = 1e-5  plane and joint sums (stats, position partials, bn_part, z_part, d_part), each
              kind as its own vector.
Without the affine the output and the input gradient are also bit-equal to the float32
oracle (oracle/shift_oracle.py); the finalized gx / gy are compared exactly (_check_pos).
dgamma / dbeta of sgcn_bn_bwd_finalize_gbn hold to 1e-5 of their largest value, its
coefficients to E5 per row.
"""
import math

import numpy as np
import pytest
import torch

from oracle import shift_oracle as so
from oracle import stream_cases as sc
from oracle import tshift_cases as tc
from oracle import tshift_ref as tr
from test_gpu_stream_ref import E5, SUM, _check, _check_sums

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7FC12345      # a quiet NaN with a payload: any rewrite of it shows in the bits
MARGIN = 32                # elements of sentinel either side of every allocation


def _id(c):
    return "x".join(map(str, c[0])) + f"-s{c[1]}" if isinstance(c[0], tuple) else \
        "x".join(map(str, c))


def _dev(t):
    """``t`` on the device as a contiguous slice of NaN storage."""
    if t is None:
        return None
    n = t.numel()
    buf = torch.full((n + 2 * MARGIN,), float("nan"), device=DEV, dtype=t.dtype)
    buf[MARGIN:MARGIN + n] = t.reshape(-1).to(DEV)
    return buf[MARGIN:MARGIN + n].view(t.shape)


class _Guarded:
    """Stands in for ``torch`` inside shiftgcn.ops while a call runs: every tensor the call
    allocates (``torch.empty`` / ``empty_like``) sits, at its exact extent, between two
    margins of the sentinel, and is itself pre-filled with it."""

    def __init__(self):
        self.allocs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, device=None, dtype=torch.float32):
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else size
        n = math.prod(size)
        buf = torch.empty((n + 2 * MARGIN,), device=device, dtype=dtype)
        buf.view(torch.int32).fill_(SENTINEL)
        self.allocs.append((buf, n))
        return buf[MARGIN:MARGIN + n].view(size)

    def empty_like(self, t):
        return self.empty(tuple(t.shape), device=t.device, dtype=t.dtype)

    def assert_margins(self, what):
        for buf, n in self.allocs:
            w = buf.element_size() // 4
            m = buf.view(torch.int32)
            assert bool((m[:MARGIN * w] == SENTINEL).all()
                        and (m[(MARGIN + n) * w:] == SENTINEL).all()), \
                f"{what}: written outside a {n}-element output"

    def assert_nothing_written(self, what):
        for buf, n in self.allocs:
            assert bool((buf.view(torch.int32) == SENTINEL).all()), f"{what}: an output was written"


class _guard:
    """``with _guard(what) as g``: shiftgcn.ops allocates through a :class:`_Guarded`; the
    margins are checked on a clean exit."""

    def __init__(self, what):
        self.what, self.g = what, _Guarded()

    def __enter__(self):
        from shiftgcn import ops
        self.real, ops.torch = ops.torch, self.g
        return self.g

    def __exit__(self, et, ev, tb):
        from shiftgcn import ops
        ops.torch = self.real
        if et is None:
            self.g.assert_margins(self.what)


def _f32_fwd(inp, xpos, ypos, stride):
    ye = so.effective_ypos(ypos.numpy(), stride)
    return torch.from_numpy(so.shift_forward(inp.numpy(), xpos.numpy(), ye, stride))


def _f32_gin(gout, xpos, ypos, H, stride):
    ye = so.effective_ypos(ypos.numpy(), stride)
    return torch.from_numpy(so.shift_bottom_backward(gout.numpy(), xpos.numpy(), ye, H, stride))


def _bit_equal(got, want):
    return torch.equal(got.cpu(), want)


# --------------------------------------------------------------------------------------
# sgcn_tshift_fwd
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.FWD_CASES, ids=_id)
def test_tshift_fwd(case):
    from shiftgcn import ops
    shape, stride = case
    B, C, H, W = shape
    Ho = H // stride
    for variant in range(tc.n_variants(C)):
        inp, xpos, ypos, scale, shift = tc.fwd_inputs(shape, variant, stride)
        d_inp, d_x, d_y, d_sc, d_sh = map(_dev, (inp, xpos, ypos, scale, shift))
        for aff in (False, True):
            ref, ref_st = tr.tshift_fwd(inp, xpos, ypos, stride, scale if aff else None,
                                        shift if aff else None)
            exact = None if aff else _f32_fwd(inp, xpos, ypos, stride)
            for stats in (False, True):
                tag = f"tshift_fwd v{variant} aff{int(aff)} stats{int(stats)}"
                with _guard(tag) as g:
                    st = g.empty((B * C * 2,), device=DEV) if stats else None
                    out = ops.tshift_fwd(d_inp, d_x, d_y, stride, d_sc if aff else None,
                                         d_sh if aff else None, stats=st)
                assert out.shape == (B, C, Ho, W)
                if Ho == 0:      # nothing is launched, nothing written
                    g.assert_nothing_written(tag)
                    continue
                _check(out, ref.to(DEV), E5, tag)
                if exact is not None:
                    assert _bit_equal(out, exact), tag + ": not bit-equal to the float32 oracle"
                if stats:
                    _check_sums(st, ref_st.to(DEV), tag + " stats")


# --------------------------------------------------------------------------------------
# sgcn_tshift_bwd
# --------------------------------------------------------------------------------------
def _check_pos(part, gx, gy, ref, tag):
    """``part`` (the per-plane partials, or None) under SUM; the finalized gx / gy exactly
    equal to the constraint of the fp64 batch mean on every channel gy_unsafe keeps, at most
    one channel left out (tests/test_oracle_tshift.py: the seeds leave none out)."""
    _, ref_part, _, ref_gx, ref_gy, ref_mean = ref[:6]
    if part is not None:
        _check_sums(part, ref_part.to(DEV), tag + " pos_part")
    skip = sc.gy_unsafe(ref_part, ref_mean)
    assert int(skip.sum()) <= 1, (tag, skip)
    keep = ~skip
    for got, want in ((gy, ref_gy), (gx, ref_gx)):
        assert torch.equal(got.cpu()[keep], want.to(got.dtype)[keep]), (tag, got, want)


class _Stats:
    """The fields of an ops.BnStats a shift backward reads."""

    batch = True

    def __init__(self, mean, invstd, scale=None, shift=None):
        self.mean, self.invstd, self.scale, self.shift = mean, invstd, scale, shift


@pytest.mark.parametrize("case", tc.BWD_CASES, ids=_id)
def test_tshift_bwd(case):
    from shiftgcn import ops
    shape, stride = case
    B, C, H, W = shape
    for variant in range(tc.n_variants(C)):
        k = tc.bwd_inputs(shape, variant, stride)
        d = {n: _dev(v) for n, v in k.items()}
        assert sc.has_all_signs(k["inp"]) or k["inp"].numel() < 8
        exact = _f32_gin(k["gout"], k["xpos"], k["ypos"], H, stride)
        exact_m = torch.where(k["inp"] > 0, exact, torch.zeros_like(exact))
        bst = _Stats(d["bn_mean"], d["bn_invstd"])
        for aff in (False, True):
            a = dict(scale=k["scale"], shift=k["shift"]) if aff else {}
            da = dict(scale=d["scale"], shift=d["shift"]) if aff else {}
            for relu in (False, True):
                ref = tr.tshift_bwd(k["gout"], k["inp"], k["xpos"], k["ypos"], stride,
                                    relu_mask=relu, bn_mean=k["bn_mean"],
                                    bn_invstd=k["bn_invstd"], **a)
                for bn in (False, True):
                    tag = f"tshift_bwd v{variant} aff{int(aff)} relu{int(relu)} bn{int(bn)}"
                    kw = dict(relu_mask=relu, bn_stats=bst if bn else None, **da)
                    with _guard(tag):
                        res = ops.tshift_bwd(d["gout"], d["inp"], d["xpos"], d["ypos"], stride,
                                             defer_pos=True, **kw)
                        gin, pp = res[0], res[1]
                        gx = torch.empty((C,), device=DEV)
                        gy = torch.empty((C,), device=DEV)
                        pp.finalize(gx, gy)
                    assert res[2] is None and len(res) == (4 if bn else 3)
                    _check(gin, ref[0].to(DEV), E5, tag + " gin")
                    assert _bit_equal(gin, exact_m if relu else exact), \
                        tag + ": gin not bit-equal to the float32 oracle"
                    assert pp.ws.numel() == 2 * B * C
                    assert torch.isfinite(pp.ws).all()
                    _check_pos(pp.ws, gx, gy, ref, tag)
                    if bn:
                        _check_sums(res[3], ref[2].to(DEV), tag + " bn_part")
                    # the finalize inside the call: the same kernels, the same bits
                    with _guard(tag + " finalized"):
                        res2 = ops.tshift_bwd(d["gout"], d["inp"], d["xpos"], d["ypos"], stride,
                                              **kw)
                    assert torch.equal(res2[0], gin) and torch.isfinite(res2[1]).all()
                    assert torch.equal(res2[1], gx) and torch.equal(res2[2], gy)
                    if bn:
                        assert torch.equal(res2[3], res[3])
        for n, v in d.items():      # no input was written
            assert torch.equal(v.cpu().view(torch.int32), k[n].view(torch.int32)), n


# --------------------------------------------------------------------------------------
# sgcn_tshift_bwd_gbn + sgcn_bn_bwd_finalize_gbn
# --------------------------------------------------------------------------------------
class _Bn:
    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


def _module_order(v, C, V):
    """local feature order (c*V + v) -> module order (v*C + c)"""
    return v.reshape(C, V).t().reshape(-1)


def _check_finalize_gbn(ops, part6, ref6, B, C, V, n_total, k, d, zmean, zinv, tag):
    """ops.bn_bwd_finalize_gbn on the kernel's six sums against the restatement on the
    reference's: dgamma / dbeta to 1e-5 of their largest value, coef to E5 per row."""
    F = C * V
    coefA = sc.t((3, C), 9100 + C, 0.5, 0.25)
    gamma = sc.t((F,), 9200 + F, 0.4, 1.0)                   # module order
    g_loc = gamma.reshape(V, C).t().reshape(-1)
    rdg, rdb, rcoef = tr.bn_bwd_finalize_gbn(ref6, n_total, coefA, k["bn_mean"], zmean, zinv,
                                             g_loc)
    bn = _Bn(_dev(gamma), _dev(sc.t((F,), 9300 + F)))
    with _guard(tag):
        coef, dg, db = ops.bn_bwd_finalize_gbn(
            part6, B, C, V, n_total, _dev(coefA), _Stats(d["bn_mean"], None),
            _Stats(_dev(zmean), _dev(zinv)), bn)
    _check(dg, _module_order(rdg, C, V).to(DEV), 1e-5, tag + " dgamma")
    _check(db, _module_order(rdb, C, V).to(DEV), 1e-5, tag + " dbeta")
    for j in range(3):
        _check(coef[j], rcoef[j].to(DEV), E5, tag + f" coef[{j}]")


@pytest.mark.parametrize("shape", tc.GBN_SHAPES, ids=_id)
def test_tshift_bwd_gbn(shape):
    from shiftgcn import ops
    B, C, H, W = shape
    fits = ops.ra_fits(H * W, W)
    assert fits == (tc.gbn_form(H, W, False) != "refuse") == (tc.gbn_form(H, W, True) != "refuse")
    for variant in range(tc.n_variants(C)):
        k = tc.bwd_inputs(shape, variant, 1)
        d = {n: _dev(v) for n, v in k.items()}
        st = _Stats(d["bn_mean"], d["bn_invstd"], d["scale"], d["shift"])
        zst, dst = _Stats(d["z_mean"], d["z_invstd"]), _Stats(d["d_mean"], d["d_invstd"])
        if not fits:
            for down in (None, (d["d"], dst)):
                with pytest.raises(ValueError, match="invalid argument"):
                    with _guard("refused") as g:
                        ops.tshift_bwd_gbn(d["gout"], d["inp"], d["xpos"], d["ypos"], st, d["z"],
                                           zst, defer_pos=True, down=down)
                g.assert_nothing_written("tshift_bwd_gbn refused")
            return
        ref = tr.tshift_bwd_gbn(k["gout"], k["inp"], k["xpos"], k["ypos"], k["scale"],
                                k["shift"], k["bn_mean"], k["bn_invstd"], k["z"], k["z_mean"],
                                k["z_invstd"], k["d"], k["d_mean"], k["d_invstd"])
        plain = ops.tshift_bwd(d["gout"], d["inp"], d["xpos"], d["ypos"], 1, scale=d["scale"],
                               shift=d["shift"], bn_stats=st)
        for down in (False, True):
            tag = f"tshift_bwd_gbn v{variant} down{int(down)}"
            with _guard(tag):
                res = ops.tshift_bwd_gbn(d["gout"], d["inp"], d["xpos"], d["ypos"], st, d["z"],
                                         zst, defer_pos=True,
                                         down=(d["d"], dst) if down else None)
                gx, gy = torch.empty((C,), device=DEV), torch.empty((C,), device=DEV)
                res[1].finalize(gx, gy)
            assert len(res) == (6 if down else 5) and res[2] is None
            assert torch.equal(res[0], plain[0]), tag + ": gin differs from sgcn_tshift_bwd"
            _check(res[0], ref[0].to(DEV), E5, tag + " gin")
            _check_pos(res[1].ws, gx, gy, ref, tag)
            _check_sums(res[3], ref[2].to(DEV), tag + " bn_part")
            z6 = res[4].view(6, B, C, W)
            for j in range(6):
                _check(z6[j], ref[6][j].to(DEV), SUM, tag + f" z_part[{j}]")
            _check_finalize_gbn(ops, res[4], ref[6], B, C, W, B * H, k, d, k["z_mean"],
                                k["z_invstd"], tag + " finalize z")
            if down:
                d6 = res[5].view(6, B, C)
                for j in range(6):
                    _check(d6[j], ref[7][j].to(DEV), SUM, tag + f" d_part[{j}]")
                _check_finalize_gbn(ops, res[5], ref[7], B, C, 1, B * H * W, k, d, k["d_mean"],
                                    k["d_invstd"], tag + " finalize d")
            # the finalize inside the call
            with _guard(tag + " finalized"):
                res2 = ops.tshift_bwd_gbn(d["gout"], d["inp"], d["xpos"], d["ypos"], st, d["z"],
                                          zst, down=(d["d"], dst) if down else None)
            assert torch.equal(res2[1], gx) and torch.equal(res2[2], gy)
            assert all(torch.equal(u, v) for u, v in zip(res2[3:], res[3:]))
        for n, v in d.items():
            assert torch.equal(v.cpu().view(torch.int32), k[n].view(torch.int32)), n


# --------------------------------------------------------------------------------------
# sgcn_tshift_pos_finalize on hand-made partials
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 70])
def test_pos_finalize(B):
    from shiftgcn import ops
    for C in (1, 3, 4, 5, 67):
        part = tc.finalize_inputs(B, C)
        rgx, rgy, mean = tr.pos_finalize(part)
        assert not sc.gy_unsafe(part.double(), mean).any()
        g = _Guarded()
        gx, gy = g.empty((C,), device=DEV), g.empty((C,), device=DEV)
        ops.PosPartials(_dev(part).reshape(-1), B, C).finalize(gx, gy)
        g.assert_margins(f"pos_finalize B{B} C{C}")
        assert torch.equal(gy.cpu(), rgy.float()), (B, C, gy, rgy)
        assert torch.equal(gx.cpu(), rgx.float()), (B, C, gx, rgx)
        assert float(gy[0]) == np.float32(1e-4) and float(gx[0]) == 0.0


# --------------------------------------------------------------------------------------
# float64 entry points
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.F64_CASES, ids=_id)
def test_tshift_f64(case):
    from shiftgcn import ops
    shape, stride = case
    B, C, H, W = shape
    for variant in range(tc.n_variants(C)):
        k = tc.bwd_inputs(shape, variant, stride)
        gout, inp = k["gout"].double(), k["inp"].double()
        xpos, ypos = k["xpos"].double(), k["ypos"].double()
        ye = so.effective_ypos(ypos.numpy(), stride)
        with _guard("tshift_fwd f64"):
            out = ops.tshift_fwd(_dev(inp), _dev(xpos), _dev(ypos), stride)
        want = torch.from_numpy(so.shift_forward(inp.numpy(), xpos.numpy(), ye, stride))
        assert out.dtype == torch.float64 and _bit_equal(out, want)
        with _guard("tshift_bwd f64"):
            gin, gx, gy = ops.tshift_bwd(_dev(gout), _dev(inp), _dev(xpos), _dev(ypos), stride)
        want = torch.from_numpy(so.shift_bottom_backward(gout.numpy(), xpos.numpy(), ye, H, stride))
        assert gin.dtype == torch.float64 and _bit_equal(gin, want)
        ref = tr.tshift_bwd(gout, inp, k["xpos"], k["ypos"], stride)
        _check_pos(None, gx, gy, ref, f"tshift_bwd f64 v{variant}")


# --------------------------------------------------------------------------------------
# refusals: argument checks, nothing enqueued
# --------------------------------------------------------------------------------------
def test_refusals():
    from shiftgcn import _lib, ops
    shape = (2, 3, 22, 25)
    B, C, H, W = shape
    k = tc.bwd_inputs(shape, 0, 1)
    d = {n: _dev(v) for n, v in k.items()}
    st = _Stats(d["bn_mean"], d["bn_invstd"], d["scale"], d["shift"])
    g3 = _dev(sc.t((B, C, H // 3, W), 1))
    calls = {
        "stride 3": lambda: ops.tshift_bwd(g3, d["inp"], d["xpos"], d["ypos"], 3),
        "scale only": lambda: ops.tshift_bwd(d["gout"], d["inp"], d["xpos"], d["ypos"], 1,
                                             scale=d["scale"]),
        "shift only": lambda: ops.tshift_bwd(d["gout"], d["inp"], d["xpos"], d["ypos"], 1,
                                             shift=d["shift"]),
        "fwd scale only": lambda: ops.tshift_fwd(d["inp"], d["xpos"], d["ypos"], 1,
                                                 scale=d["scale"]),
        "bn_part without statistics": lambda: ops.tshift_bwd(
            d["gout"], d["inp"], d["xpos"], d["ypos"], 1, bn_stats=_Stats(None, None)),
    }
    for what, call in calls.items():
        with pytest.raises(ValueError, match="invalid argument"):
            with _guard(what) as g:
                call()
        assert g.allocs, what
        g.assert_nothing_written(what)
    # W = 65 for the GBN form
    wide = (1, 2, 9, 65)
    kw = tc.bwd_inputs(wide, 0, 1)
    dw = {n: _dev(v) for n, v in kw.items()}
    assert not ops.ra_fits(9 * 65, 65) and tc.bwd_form(9, 65, 1)[0] == "global"
    with pytest.raises(ValueError, match="invalid argument"):
        with _guard("W65") as g:
            ops.tshift_bwd_gbn(dw["gout"], dw["inp"], dw["xpos"], dw["ypos"],
                               _Stats(dw["bn_mean"], dw["bn_invstd"], dw["scale"], dw["shift"]),
                               dw["z"], _Stats(dw["z_mean"], dw["z_invstd"]))
    g.assert_nothing_written("gbn W = 65")
    # a workspace one byte short (ops sizes its own: the C entry point directly)
    lib = _lib.load()
    g = _Guarded()
    gin, gx, gy = g.empty(shape, device=DEV), g.empty((C,), device=DEV), g.empty((C,), device=DEV)
    ws = g.empty((2 * B * C,), device=DEV)
    nbytes = lib.sgcn_tshift_bwd_ws_bytes(B, C)
    assert nbytes == 8 * B * C
    p = ops._ptr
    args = lambda nb: (p(d["gout"]), p(d["inp"]), p(d["xpos"]), p(d["ypos"]), None, None, 0,
                       None, None, None, p(gin), p(gx), p(gy), p(ws), nb, B, C, H, W, 1, 1,
                       ops._stream(gin))
    with pytest.raises(ValueError, match="invalid argument"):
        _lib.check(lib.sgcn_tshift_bwd(*args(nbytes - 1)), "sgcn_tshift_bwd")
    g.assert_nothing_written("short workspace")
    _lib.check(lib.sgcn_tshift_bwd(*args(nbytes)), "sgcn_tshift_bwd")       # exact size: runs
    g.assert_margins("exact workspace")
    ref = tr.tshift_bwd(k["gout"], k["inp"], k["xpos"], k["ypos"], 1)
    _check(gin, ref[0].to(DEV), E5, "exact workspace gin")
    _check_pos(ws, gx, gy, ref, "exact workspace")
