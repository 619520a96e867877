"""Pin the float64 restatements of the contraction entry points (oracle/pw_ref.py) without
a GPU: against F.conv2d and its autograd weight / bias / input gradients, and against the
reference's index_select shift_in / shift_out gathers (oracle/model_oracle.py); check that
the shape tables of tests/test_gpu_pw_ref.py reach every launch form a contraction can reach
(oracle/pw_cases.py mirrors the host choosers), that the mirrors' split counts are the built
library's, and that the entry points refuse bad arguments before any launch."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import model_oracle as mo
from oracle import pw_cases as pc
from oracle import pw_ref as pr
from oracle import torch_shift as ts

F64 = torch.float64
TOL = 1e-12


def _r(shape, seed, scale=1.0):
    return pc.rnd(shape, seed, scale).double()


def _close(a, b, tol=TOL):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= tol * (float(b.abs().max()) + 1e-300)


# --------------------------------------------------------------------------------------
# pw_ref against conv2d + autograd
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tstride", [1, 2])
@pytest.mark.parametrize("relu", [False, True])
def test_plain_forward_and_gradients_match_conv2d(tstride, relu):
    B, K, M, T, V = 3, 5, 7, 6, 4
    To = (T - 1) // tstride + 1
    x = _r((B, K, T, V), 1).requires_grad_(True)
    w = _r((M, K), 2).requires_grad_(True)
    bias = _r((M,), 3).requires_grad_(True)
    dy = _r((B, M, To, V), 4)
    a = F.conv2d(x, w.view(M, K, 1, 1), bias, stride=(tstride, 1))
    y_t = torch.relu(a) if relu else a
    y_t.backward(dy)

    xd, wd, bd = x.detach(), w.detach(), bias.detach()
    y = torch.full((B, M, To, V), 9.0, dtype=F64)
    flat, idx = pr.pw_fwd_ref(wd, False, bd, pr.Plane(xd, tstride), pr.Plane(y), M, K, To, V,
                              relu=relu)
    assert _close(flat[idx], y_t) and _close(flat.view_as(y), y_t)
    # m-contiguous weights + accumulate into the previous contents
    flat2, _ = pr.pw_fwd_ref(wd.t().contiguous(), True, bd, pr.Plane(xd, tstride), pr.Plane(y),
                             M, K, To, V, relu=relu, accumulate=True)
    assert _close(flat2.view_as(y), y_t.detach() + 9.0)
    # no bias
    flat3, _ = pr.pw_fwd_ref(wd, False, None, pr.Plane(xd, tstride), pr.Plane(y), M, K, To, V)
    assert _close(flat3.view_as(y), a.detach() - bd.view(1, M, 1, 1))

    g = torch.where(y_t.detach() > 0, dy, torch.zeros_like(dy)) if relu else dy
    old_w, old_b = _r((M, K), 5), _r((M,), 6)
    dw, db = pr.pw_dw_ref(pr.Plane(g), pr.Plane(xd, tstride), M, K, To, V)
    assert _close(dw, w.grad) and _close(db, bias.grad)
    dwt, dba = pr.pw_dw_ref(pr.Plane(g), pr.Plane(xd, tstride), M, K, To, V, transpose=True,
                            dw_old=old_w.t().contiguous(), dbias_old=old_b)
    assert _close(dwt, (w.grad + old_w).t()) and _close(dba, bias.grad + old_b)
    # dX: the same contraction with w read transposed (A'[k][m] = w[m*K + k]), scattered
    # to every tstride-th row of a zeroed gradient, accumulating
    dx = torch.zeros(B, K, T, V, dtype=F64)
    fx, ix = pr.pw_fwd_ref(wd, True, None, pr.Plane(g), pr.Plane(dx, tstride), K, M, To, V,
                           accumulate=True)
    assert _close(fx.view_as(dx), x.grad)
    assert ix.numel() == B * K * To * V and ix.unique().numel() == ix.numel()


@pytest.mark.parametrize("C,D,V", [(5, 7, 4), (9, 3, 4), (3, 2, 1)])
@pytest.mark.parametrize("sign", [+1, -1])
def test_rotated_masked_forms_match_the_reference_gathers(C, D, V, sign):
    """Shift_gcn.forward (shift_gcn.py:125-136; oracle/model_oracle.py) with its
    index_select shift_in / shift_out (sign = +1) or the two index tables swapped (sign =
    -1: the opposite rotations), and its autograd gradients."""
    n, t = 2, 3
    x0 = _r((n, C, t, V), 11).requires_grad_(True)
    fmask = _r((1, V, C), 12, 0.5).requires_grad_(True)
    W = _r((C, D), 13).requires_grad_(True)
    lb = _r((1, 1, D), 14).requires_grad_(True)
    dy = _r((n, D, t, V), 15)
    s_in = torch.from_numpy(mo.spatial_shift_indices(V, C, sign))
    s_out = torch.from_numpy(mo.spatial_shift_indices(V, D, -sign))
    x = x0.permute(0, 2, 3, 1).contiguous().view(n * t, V * C)
    x = torch.index_select(x, 1, s_in).view(n * t, V, C)
    xg = x * (torch.tanh(fmask) + 1)
    xg.retain_grad()
    z = torch.einsum("nwc,cd->nwd", xg, W).contiguous() + lb
    z = torch.index_select(z.view(n * t, -1), 1, s_out)
    y_t = z.view(n, t, V, D).permute(0, 3, 1, 2)
    y_t.backward(dy)

    m = (torch.tanh(fmask) + 1).detach().view(V, C)
    y = torch.zeros(n, D, t, V, dtype=F64)
    flat, idx = pr.pw_fwd_ref(W.detach(), True, lb.detach().view(D), pr.Plane(x0.detach(), 1, sign),
                              pr.Plane(y, 1, sign), D, C, t, V, mask=m)
    assert _close(flat.view_as(y), y_t)
    dw, db = pr.pw_dw_ref(pr.Plane(dy, 1, sign), pr.Plane(x0.detach(), 1, sign), D, C, t, V,
                          mask=m, transpose=True)
    assert _close(dw, W.grad) and _close(db, lb.grad.view(D))
    # the gathered-and-masked operand's gradient: w read as (C, D) k-contiguous
    dxt = torch.zeros(n, C, t, V, dtype=F64)
    fx, _ = pr.pw_fwd_ref(W.detach(), False, None, pr.Plane(dy, 1, sign), pr.Plane(dxt), C, D, t, V)
    want = xg.grad.view(n, t, V, C).permute(0, 3, 1, 2)
    assert _close(fx.view_as(dxt), want)
    # and through the mask and the gather's transpose, x0's gradient
    got = pr.Plane(x0.grad, 1, sign).read(n, C, t, V)
    assert _close(fx.view_as(dxt) * m.t().reshape(1, C, 1, V), got)


def test_plane_addressing_of_a_view():
    """A channel / batch slice and the odd rows of a larger tensor: read and written inside
    the larger storage, nothing else touched."""
    big = _r((4, 9, 10, 5), 21)
    B, C, T, V = 2, 3, 5, 5
    view = big[1:3, 2:5, 1:]
    p = pr.Plane(view, 2, -1)
    got = p.read(B, C, T, V)
    c = torch.arange(C).view(C, 1)
    v = torch.arange(V).view(1, V)
    want = big[1:3, 2:5, 1::2].gather(3, ((v - c) % V).view(1, C, 1, V).expand(B, C, T, V))
    assert torch.equal(got, want)
    w = _r((C, 2), 22)
    flat, idx = pr.pw_fwd_ref(w, False, None, pr.Plane(_r((B, 2, T, V), 23)), p, C, 2, T, V)
    untouched = torch.ones(flat.numel(), dtype=torch.bool)
    untouched[idx.reshape(-1)] = False
    assert int((~untouched).sum()) == B * C * T * V
    assert torch.equal(flat[untouched], big.reshape(-1)[untouched])


def test_tshift_ref_is_shift_then_contraction():
    B, K, M, T, V = 2, 5, 3, 9, 4
    x = pc.rnd((B, K, T, V), 31)
    w, bias = pc.rnd((M, K), 32), pc.rnd((M,), 33)
    scale, shift = pc.rnd((K,), 34) + 2, pc.rnd((K,), 35)
    xpos = torch.tensor([0.0, 1e-8, -1.5, 1.0, -2.25])
    ypos = torch.tensor([0.5, -3.5, 2.0, 11.0, -0.75])
    y = torch.zeros(B, M, T, V)
    flat, idx, S = pr.pw_fwd_tshift_ref(w, bias, pr.Plane(x), xpos, ypos, scale, shift,
                                        pr.Plane(y), M, K, T, V, relu=True)
    aff = x.double() * scale.double().view(1, K, 1, 1) + shift.double().view(1, K, 1, 1)
    S_t = ts.shift_forward(aff, xpos.double(), ypos.double(), 1)
    assert _close(S, S_t)
    want = torch.relu(F.conv2d(S_t, w.double().view(M, K, 1, 1), bias.double()))
    assert _close(flat.view_as(y), want)


# --------------------------------------------------------------------------------------
# coverage of the launch forms
# --------------------------------------------------------------------------------------
SIZES = range(1, 301)


def _dw_key(f):
    return (f["family"], f["tile"])


def test_dw_table_reaches_every_reachable_family_and_tile():
    reach = {_dw_key(pc.dw_form(2, M, Nc, 7, 25)) for M in SIZES for Nc in SIZES}
    want = ({("dw", t) for t in itertools.product((64, 128), repeat=2)} |
            {("dw3", (128, 128)), ("dw3", (256, 128)), ("dw3", (256, 256))} |
            {("smallc", (n,)) for n in (1, 2, 3, 4)})
    assert reach == want      # no smaller pw_dw3_kernel tile: use_dw3 needs M * Nc >= 128 * 128
    table = {_dw_key(pc.dw_form(*c)) for c in pc.DW_TABLE}
    assert table == want
    assert set(pc.DW_FLAG_SHAPES) <= want
    for (fam, tile), shapes in pc.DW_FLAG_SHAPES.items():
        for c in shapes:
            assert c in pc.DW_TABLE
            f = pc.dw_form(*c)
            assert f["family"] == fam and (fam == "smallc" or f["tile"] == tile), c


def test_dw_unreachable_forms():
    """The module docstring's list, by enumeration (the split geometry does not enter)."""
    for M in SIZES:
        for Nc in SIZES:
            f = pc.dw_form(2, M, Nc, 7, 25)
            if f["family"] == "dw3" and f["tile"] == (128, 128):
                assert (M, Nc) == (128, 128)
            if f["family"] == "dw" and f["tile"] == (128, 128):
                assert not f["fast"]
            if f["family"] == "dw":
                assert Nc > pc.K_DWC_MAX_C and M * Nc < pc.K_DW3_MIN
            if Nc <= pc.K_DWC_MAX_C:
                assert f["family"] == "smallc"
    # smallc: an empty split only from 256 positions per split up
    for M in (1, 64, 65, 100, 300):
        for P in list(range(1, 3000)) + [131199, 131200, 131201, 262144, 300000]:
            S = pc.dwc_splits(M, P)
            per = -(-P // S)
            if per < 256:
                assert (S - 1) * per < P, (M, P)


def test_dw_table_operand_forms_and_split_geometry():
    forms = [pc.dw_form(*c, mask=mk and c[4] <= pc.K_MASK_MAX_V, g_rsign=gr, x_rsign=xr,
                        dbias=True)
             for c in pc.DW_TABLE for gr, xr, mk in pc.DW_OPERANDS]
    # pw_dw_kernel: mask / plain / general per tile, and the fast path wherever it exists
    for tile in itertools.product((64, 128), repeat=2):
        got = {f["flags"] for f in forms if f["family"] == "dw" and f["tile"] == tile}
        assert got == {"mask", "plain", "general"}, tile
        assert any(f["fast"] for f in forms if f["family"] == "dw" and f["tile"] == tile) == \
            (tile != (128, 128))
        if tile != (128, 128):   # the incremental advance: > 1 chunk per split, over a sample end
            assert any(f["fast"] and f["per"] > 1 and f["wraps"] for f in forms
                       if f["family"] == "dw" and f["tile"] == tile), tile
    for fam in ("dw", "dw3", "smallc"):
        mine = [f for f in forms if f["family"] == fam]
        assert any(f["steps"] > 1 for f in mine), fam
        assert any(f["empty"] > 0 for f in mine), fam
        assert any(f["mid"] for f in mine), fam
        assert any(f["wraps"] for f in mine), fam
    for tile in ((128, 128), (256, 128), (256, 256)):
        mine = [f for f in forms if f["family"] == "dw3" and f["tile"] == tile]
        assert any(f["steps"] > 1 and f["empty"] > 0 for f in mine), tile
        assert any(f["cross"] for f in mine), tile
    assert any(f.get("ragged_last") and f["steps"] > 1 for f in forms if f["family"] == "dw3")
    assert any(f["family"] == "smallc" and f["per"] >= 256 and f["empty"] for f in forms)
    # the V edges of the table
    vs = {c[4] for c in pc.DW_TABLE}
    assert {1, 25, 33, 64} <= vs and max(vs) > pc.K_MASK_MAX_V
    # slab reduce beyond the old tests' S = 107, and its 256-split unrolled loop
    assert max(f["S"] for f in forms) >= 1024


def test_dw3_flag_cross_covers_every_instance():
    for key, shapes in pc.DW_FLAG_SHAPES.items():
        if key[0] != "dw3":
            continue
        for c in shapes:
            assert c[4] <= pc.K_MASK_MAX_V
            got = {pc.dw_form(*c, mask=mk, g_rsign=gr, x_rsign=xr, dbias=db)["flags"]
                   for mk in (False, True) for gr in pc.RSIGNS for xr in pc.RSIGNS
                   for db in (False, True)}
            assert got == set(itertools.product((False, True), repeat=4)), c


def test_forward_tables_reach_every_form():
    flags4 = set(itertools.product((False, True), repeat=4))
    want = {("pwg", tile, st, fl) for (tile, st) in pc.FWD_FLAG_PAIRS for fl in flags4}
    want |= {("smallm", None, None, fl) for fl in itertools.product((False, True), repeat=2)}
    reach = {pc.fwd_form(M, K, mk, xr, yr, amc, acc)
             for M in SIZES for K in range(1, pc.K_MAX_K + 1) for mk in (False, True)
             for xr in (0, 1) for yr in (0, 1) for amc in (False, True) for acc in (False, True)}
    assert reach == want      # A-resident on 64 x 256 only; smallm never masked or rotated
    got = {pc.fwd_case_form(c) for c in pc.fwd_flag_cases()}
    assert got == want
    # every tile sees both signs on both operands
    for key, (M, K) in pc.FWD_FLAG_PAIRS.items():
        seen = {(c["x_rsign"], c["y_rsign"]) for c in pc.fwd_rsign_cases()
                if (c["M"], c["K"]) == (M, K)}
        assert seen == set(itertools.product(pc.RSIGNS, repeat=2))
        assert pc.fwd_form(M, K, True, 1)[1:3] == key
    # the (M, K) pairs: each (tile, staging) with ragged M, ragged K, and its boundaries
    by = {}
    for M, K in pc.FWD_PAIRS:
        f = pc.fwd_form(M, K)
        by.setdefault(f[:3], []).append((M, K))
    assert set(by) == {k[:3] for k in want}
    for key, pairs in by.items():
        if key[0] == "pwg":
            assert any(M % 32 for M, _ in pairs) and any(K % 16 for _, K in pairs), key
    ms, ks = {M for M, _ in pc.FWD_PAIRS}, {K for _, K in pc.FWD_PAIRS}
    assert {1, 4, 5, 64, 65, 128, 129, 300} <= ms
    assert {1, 3, 16, 17, 64, 65, 100, 256} <= ks
    for a, b in ((5, 16), (5, 17), (64, 64), (64, 65)):    # the A-resident K window, M <= 64
        assert (a, b) in pc.FWD_PAIRS
    # planes: below one tile, an exact tile, V = 1, V = 33, V > 64, V = 64
    P = {B * T * V for B, T, V in pc.FWD_PLANES}
    assert min(P) < 128 and 256 in P
    assert {1, 25, 33, 64, 70} <= {V for _, _, V in pc.FWD_PLANES}
    # the fused temporal shift: every tile, a ragged K on each, M past 256
    tiles = {pc.tshift_form(M) for M in SIZES}
    assert tiles == {(64, 256), (128, 256), (256, 128)}
    for tile in tiles:
        mine = [c for c in pc.TSHIFT_CASES if pc.tshift_form(c[2]) == tile]
        assert any(c[1] % 16 for c in mine) and any(c[1] % 16 == 0 for c in mine), tile
    assert any(c[2] > 256 for c in pc.TSHIFT_CASES)


# --------------------------------------------------------------------------------------
# the mirrors against the built library; refusals
# --------------------------------------------------------------------------------------
def test_mirror_split_counts_are_the_librarys():
    from shiftgcn import _lib
    lib = _lib.load()
    for c in pc.DW_TABLE:
        assert lib.sgcn_pw_dw_ws_bytes(*c) == pc.dw_ws_bytes(*c), c
    for M, Nc in ((1, 1), (64, 4), (64, 5), (127, 129), (128, 128), (129, 128), (300, 300)):
        for B, T, V in ((1, 1, 1), (2, 300, 25), (32, 75, 25), (64, 300, 33)):
            assert lib.sgcn_pw_dw_ws_bytes(B, M, Nc, T, V) == pc.dw_ws_bytes(B, M, Nc, T, V)


_PTR = ctypes.c_void_p(4096)    # a non-NULL address no refused call may touch


def _fwd(lib, *, mask=None, B=0, M=8, K=8, T=4, V=5, xb=160, xc=20, xt=1, xr=0, yb=160, yc=20,
         yt=1, yr=0):
    return lib.sgcn_pw_fwd(_PTR, 0, None, _PTR, xb, xc, xt, xr, mask, _PTR, yb, yc, yt, yr, 0,
                           0, B, M, K, T, V, None)


def _tsh(lib, *, B=0, M=8, K=8, T=4, V=5, xc=20, yc=20, ws_bytes=1 << 20, two_row=0):
    return lib.sgcn_pw_fwd_tshift(_PTR, None, _PTR, K * xc, xc, _PTR, _PTR, None, None, None,
                                  _PTR, ws_bytes, _PTR, M * yc, yc, 0, two_row, B, M, K, T, V,
                                  None)


def _dw(lib, *, mask=None, B=2, M=8, Nc=8, T=4, V=5, gt=1, gr=0, xt=1, xr=0, gc=20, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.sgcn_pw_dw_ws_bytes(B, M, Nc, T, V)
    return lib.sgcn_pw_dw(_PTR, M * gc, gc, gt, gr, _PTR, Nc * 20, 20, xt, xr, mask, _PTR, 0, 0,
                          None, 0, _PTR, ws_bytes, B, M, Nc, T, V, None)


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below is rejected by the argument checks alone: forward calls carry B = 0
    or T = 0, at which a WELL-formed call returns 0 without touching a pointer (asserted
    first), so SGCN_EINVAL comes from the named argument."""
    from shiftgcn import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    assert _fwd(lib) == 0 and _fwd(lib, B=3, T=0) == 0 and _fwd(lib, mask=_PTR, V=64) == 0
    assert _tsh(lib) == 0 and _tsh(lib, B=3, T=0) == 0 and _tsh(lib, two_row=2) == 0
    assert _fwd(lib, K=256) == 0 and _fwd(lib, K=257) == E
    assert _tsh(lib, K=256) == 0 and _tsh(lib, K=257) == E
    assert _fwd(lib, mask=_PTR, V=65) == E
    for r in (2, -2):
        assert _fwd(lib, xr=r) == E and _fwd(lib, yr=r) == E
    assert _fwd(lib, xt=0) == E and _fwd(lib, yt=0) == E
    # an operand extent of 2^29 elements (K * cstride alone; K * cstride < 2^31 holds)
    assert _fwd(lib, B=1, T=0, K=128, xc=(1 << 22) - 1) == 0
    assert _fwd(lib, B=1, T=0, K=128, xc=1 << 22) == E
    assert _fwd(lib, B=1, T=0, M=128, yc=1 << 22) == E
    assert _tsh(lib, B=1, T=0, K=128, xc=1 << 22) == E
    assert _tsh(lib, two_row=3) == E and _tsh(lib, two_row=-1) == E
    assert _tsh(lib, xc=19) == E and _tsh(lib, yc=19) == E      # cstride < T * V
    # B > 0: the workspace check comes after the pointers, before any launch
    assert _tsh(lib, B=2, ws_bytes=lib.sgcn_pw_tshift_ws_bytes(8) - 1) == E
    # the weight gradient has no empty form: B = 0 and T = 0 are refused themselves
    assert _dw(lib, B=0) == E and _dw(lib, T=0) == E
    assert _dw(lib, ws_bytes=lib.sgcn_pw_dw_ws_bytes(2, 8, 8, 4, 5) - 1) == E
    assert _dw(lib, mask=_PTR, V=65) == E
    assert _dw(lib, gt=0) == E and _dw(lib, xt=0) == E
    for r in (2, -2):
        assert _dw(lib, gr=r) == E and _dw(lib, xr=r) == E
    assert _dw(lib, M=128, Nc=128, gc=1 << 22) == E             # pw_dw3: extent 2^29
