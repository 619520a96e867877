"""shift_in's input gradient inside a unit is never stored (fused.DA_REFORM).

The GBN shift_in backward keeps its sums only (sgcn_tshift_bwd_gbn with gin = NULL) and the gcn
BatchNorm backward apply re-forms the gradient from the staged gout plane
(sgcn_bn_bwd_apply_tsh). Both kernels form the element through the same device function, so
every comparison with the pair they replace (ops.tshift_bwd_gbn + ops.bn_bwd_apply) is
``torch.equal``; the same cases are checked once against the float64 restatements
(oracle/tshift_ref.py then oracle/stream_ref.py) at the bar both ops carry there (E5: the
four-tap blend, then two affine maps with coefficients below 1).

Planes: B = 2, C = V + 2 (the in-row rotation (v - c) mod V wraps), (T, V) reaching every
(threads, elements per thread) form of the GBN chooser without and with a down conv. The
positions put on some channel: a fractional ypos in (-1, 1), 4 < |ypos| < T (past the pad rows),
|ypos| > T (every tap out of range), xpos = +-1e-8 and |xpos| >= 1 (past the pad columns).
Outputs sit in a sentinel NaN pattern between guarded margins (test_gpu_tshift_ref._guard).
"""
import pytest
import torch

import formula
from oracle import stream_cases as sc
from oracle import stream_ref as sr
from oracle import tshift_cases as tc
from oracle import tshift_ref as tr
from test_gpu_stream_ref import E5, _check
from test_gpu_tshift_ref import _Guarded, _Stats, _dev, _guard

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (T, V): 256 x 8, 256 x 16 (down: 256 x 16), 256 x 16 / 24, 256 x 32 (down: 512 x 16),
# 512 x 16 (down: 512 x 16), 512 x 20
PLANES = [(8, 25), (75, 25), (150, 25), (300, 25), (240, 33), (300, 33)]


def _positions(C, T):
    """(xpos, ypos): channels 0..8 cover the classes in the module docstring, the rest are
    fractional."""
    xp = sc.t((C,), 501, 1e-8)
    yp = sc.t((C,), 502, 0.9)
    assert float(yp.abs().max()) < 1.0 and C >= 9 and T > 5.3
    fixed = [(1e-8, 0.37), (-1e-8, -0.81), (0.0, 5.3), (1e-8, -4.6), (0.0, T + 2.5),
             (-1e-8, -(T + 1.25)), (1.3, 0.4), (-2.2, -1.1), (1.0, 0.5)]
    for c, (x, y) in enumerate(fixed):
        xp[c], yp[c] = x, y
    return xp, yp


_CASES = {}


def _case(T, V):
    """Inputs (CPU, float32) and the float64 reference of one plane, made once."""
    key = (T, V)
    if key in _CASES:
        return _CASES[key]
    B, C = 2, V + 2
    shape = (B, C, T, V)
    k = tc.bwd_inputs(shape, 0, 1)
    k["xpos"], k["ypos"] = _positions(C, T)
    k["coefZ"] = sc.t((3, C * V), 511, 0.5, 0.25)
    k["coefD"] = sc.t((3, C), 512, 0.5, 0.25)
    k["coefA"] = sc.t((3, C), 513, 0.5, 0.25)
    ref = tr.tshift_bwd_gbn(k["gout"], k["inp"], k["xpos"], k["ypos"], k["scale"], k["shift"],
                            k["bn_mean"], k["bn_invstd"], k["z"], k["z_mean"], k["z_invstd"],
                            k["d"], k["d_mean"], k["d_invstd"])
    refs = {}
    for down in (False, True):
        refs[down] = sr.bn_bwd_apply(ref[0], k["inp"], True, k["z"], k["coefZ"], 3,
                                     r=k["d"] if down else None,
                                     rcoef=k["coefD"] if down else None, want_dr=not down,
                                     dy_coef=k["coefA"])
    _CASES[key] = (k, refs)
    return _CASES[key]


def _same(a, b, what):
    """bit for bit (a sentinel NaN left in either fails: NaN != NaN)"""
    assert a.shape == b.shape and torch.equal(a, b), what


@pytest.mark.parametrize("down", [False, True], ids=["id", "down"])
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_reformed_pair_equals_stored_pair(plane, down):
    from shiftgcn import ops
    T, V = plane
    B, C = 2, V + 2
    assert ops.ra_fits(T * V, V) and tc.gbn_form(T, V, down) != "refuse"
    k, refs = _case(T, V)
    d = {n: _dev(v) for n, v in k.items()}
    st = _Stats(d["bn_mean"], d["bn_invstd"], d["scale"], d["shift"])
    zst, dst = _Stats(d["z_mean"], d["z_invstd"]), _Stats(d["d_mean"], d["d_invstd"])
    dn = (d["d"], dst) if down else None
    r, rcoef = (d["d"], d["coefD"]) if down else (None, None)
    tag = f"{T}x{V} down{int(down)}"

    def gbn(store, defer):
        with _guard(f"{tag} gbn store{int(store)} defer{int(defer)}"):
            return ops.tshift_bwd_gbn(d["gout"], d["inp"], d["xpos"], d["ypos"], st, d["z"], zst,
                                      defer_pos=defer, down=dn, store=store)

    # the stored pair
    old = gbn(True, True)
    with _guard(tag + " apply") as g:
        odr = g.empty_like(d["z"])
        odx = ops.bn_bwd_apply(old[0], d["inp"], True, d["z"], d["coefZ"], 3, r=r, rcoef=rcoef,
                               dr=odr, dy_coef=d["coefA"])
    # the sums-only launch: every partial buffer, the position partials (defer_pos) ...
    new = gbn(False, True)
    assert new[0] is None and len(new) == len(old) == (6 if down else 5)
    _same(new[1].ws, old[1].ws, tag + " position partials")
    for j, n in ((3, "bn_part"), (4, "z_part"), (5, "d_part"))[:len(old) - 3]:
        _same(new[j], old[j], f"{tag} {n}")
    # ... and the positions' gradients finalized by the call itself (the direct form)
    old_d, new_d = gbn(True, False), gbn(False, False)
    assert new_d[0] is None
    for j in range(1, len(old_d)):
        _same(new_d[j], old_d[j], f"{tag} direct [{j}]")
    _same(old_d[0], old[0], tag + " stored gin, both position forms")
    # the re-forming apply
    with _guard(tag + " apply_tsh"):
        ndx, ndr = ops.bn_bwd_apply_tsh(d["gout"], d["xpos"], d["ypos"], d["inp"], d["z"],
                                        d["coefZ"], d["coefA"], r=r, rcoef=rcoef)
    _same(ndx, odx, tag + " dZ")
    _same(ndr, odr, tag + " dr")
    # the float64 composition, once per case
    _check(ndx, refs[down][0].to(DEV), E5, tag + " dZ vs fp64")
    _check(ndr, refs[down][1].to(DEV), E5, tag + " dr vs fp64")
    for n, v in d.items():      # no input was written
        assert torch.equal(v.cpu().view(torch.int32), k[n].view(torch.int32)), n


def test_refused_plane():
    """A plane ra_fits rejects: both new forms refuse without writing anything."""
    from shiftgcn import ops
    T, V = 700, 25          # 17,500 floats: above the LDS-staged planes
    assert not ops.ra_fits(T * V, V)
    B, C = 1, 2
    shape = (B, C, T, V)
    x = _dev(sc.t(shape, 521))
    xp, yp = _dev(sc.t((C,), 522, 1e-8)), _dev(sc.t((C,), 523, 0.9))
    cz, ca = _dev(sc.t((3, C * V), 524)), _dev(sc.t((3, C), 525))
    with pytest.raises(ValueError, match="invalid argument"):
        with _guard("refused") as g:
            ops.bn_bwd_apply_tsh(x, xp, yp, x, x, cz, ca)
    g.assert_nothing_written("bn_bwd_apply_tsh refused")


# --------------------------------------------------------------------------------------
# unit and chain level: the knob on against the knob off, bit for bit
# --------------------------------------------------------------------------------------
def _t(shape, seed, scale=1.0):
    return formula.tensor(tuple(shape), seed, scale).to(DEV)


def _chain(layout, seed):
    import shiftgcn
    units = torch.nn.ModuleList(
        [shiftgcn.TCN_GCN_unit(ci, co, None, stride=s, num_point=25) for ci, co, s in layout])
    formula.fill_state(units, seed=seed)
    return units.to(DEV).train()


def _grads(units, x, weight):
    import shiftgcn
    units.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    y = xr
    with shiftgcn.shift_gcn.linked_units(list(units)):
        for u in units:
            y = u(y)
    (y * weight).sum().backward()
    torch.cuda.synchronize()
    g = {n: p.grad.clone() for n, p in units.named_parameters() if p.grad is not None}
    g["input"] = xr.grad.clone()
    return g


def _count_tsh(monkeypatch):
    from shiftgcn import ops
    calls = {"tsh": 0, "stored": 0}
    real_tsh, real_gbn = ops.bn_bwd_apply_tsh, ops.tshift_bwd_gbn

    def tsh(*a, **k):
        calls["tsh"] += 1
        return real_tsh(*a, **k)

    def gbn(*a, store=True, **k):
        calls["stored"] += bool(store)
        return real_gbn(*a, store=store, **k)

    monkeypatch.setattr(ops, "bn_bwd_apply_tsh", tsh)
    monkeypatch.setattr(ops, "tshift_bwd_gbn", gbn)
    return calls


@pytest.mark.parametrize("async_dw", [1, 0])
def test_chain_bit_identical(async_dw, monkeypatch):
    """identity, down + residual conv, identity (T = 16, V = 25, B = 2): one backward under
    each setting of the knob; every parameter gradient and the input gradient are equal."""
    from shiftgcn import fused
    monkeypatch.setattr(fused, "ASYNC_DW", async_dw)
    units = _chain([(16, 16, 1), (16, 32, 1), (32, 32, 1)], 21)
    x, w = _t((2, 16, 16, 25), 531), _t((2, 32, 16, 25), 532)
    calls = _count_tsh(monkeypatch)
    monkeypatch.setattr(fused, "DA_REFORM", 0)
    ref = _grads(units, x, w)
    assert calls == {"tsh": 0, "stored": 3}
    monkeypatch.setattr(fused, "DA_REFORM", 1)
    got = _grads(units, x, w)
    assert calls == {"tsh": 3, "stored": 3}      # every unit took the new pair
    assert ref.keys() == got.keys() and len(ref) > 30
    for n in ref:
        assert torch.equal(got[n], ref[n]), n


def test_unit_on_a_refused_plane_keeps_the_stored_gradient(monkeypatch):
    """T * V above the LDS-staged planes: with the knob on the unit still takes the looping
    kernels and the stored gradient, and matches the knob off."""
    from shiftgcn import fused, ops
    T = 700
    assert not ops.ra_fits(T * 25, 25)
    units = _chain([(4, 4, 1)], 23)
    x, w = _t((1, 4, T, 25), 541), _t((1, 4, T, 25), 542)
    calls = _count_tsh(monkeypatch)
    out = {}
    for knob in (0, 1):
        monkeypatch.setattr(fused, "DA_REFORM", knob)
        out[knob] = _grads(units, x, w)
    assert calls == {"tsh": 0, "stored": 0}
    for n in out[0]:
        assert torch.equal(out[1][n], out[0][n]), n
