"""Pre-masked and per-plane output gradients of the unit backward (fused.PREMASK).

A linked unit's output gradient may arrive with its ReLU mask already applied (stored by
the next unit's sgcn_gcn_dx_finish, SGCN_DXF_MASK_DX) or as one value per plane (the pool's
gradient), so no backward kernel reads the unit's output only for ``out > 0``. Every
consumer forms exactly ``mask ? dout : +0`` either way, so every comparison here is
``torch.equal``: kernel forms against the forms they replace, and whole backwards with the
knob on against the knob off.
"""
import pytest
import torch

import formula

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C, T, V): ragged with C % V != 0 rotations; the NTU plane (256 threads x 32); the
# MediaPipe plane (512-thread form); V > 64: the looping kernels (no LDS shift backward)
SHAPES = [(2, 5, 7, 25), (2, 4, 300, 25), (2, 3, 300, 33), (1, 2, 9, 70)]
RA_SHAPES = SHAPES[:3]


def _t(shape, seed, scale=1.0):
    return formula.tensor(tuple(shape), seed, scale).to(DEV)


def _act(shape, seed):
    """An activation-like tensor with exact zeros, positives and negatives."""
    v = _t(shape, seed)
    return torch.where(v.abs() < 0.25, torch.zeros_like(v), v)


def _stats(F, seed):
    from shiftgcn import ops
    st = ops.BnStats(F, DEV)
    st.mean.copy_(_t((F,), seed, 0.3))
    st.invstd.copy_(_t((F,), seed + 1, 0.4) + 1.0)
    st.scale.copy_(_t((F,), seed + 2, 0.5) + 1.0)
    st.shift.copy_(_t((F,), seed + 3, 0.2))
    return st


def _expand(p, shape):
    return p[:, :, None, None].expand(*shape).contiguous()


# --------------------------------------------------------------------------------------
# kernel level
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", ["plain", "add2", "identity", "identity_prev", "add1_prev"])
def test_dx_finish_masked_dx(shape, form):
    from shiftgcn import ops
    B, C, T, V = shape
    dxt, x0, m = _t(shape, 1), _act(shape, 2), _t((V, C), 3) + 1.0
    kw = {}
    if form in ("identity", "identity_prev", "add1_prev"):
        kw["add1"] = _t(shape, 4)
    if form in ("add2", "identity", "identity_prev"):
        kw["add2"] = _t(shape, 5)
    if form in ("identity", "identity_prev"):
        kw["add2_mask"] = _act(shape, 6)
    if form.endswith("_prev"):
        kw["prev"] = (_t(shape, 7), _stats(C, 8))
    plain = ops.gcn_dx_finish(dxt, x0, m, **kw)
    masked = ops.gcn_dx_finish(dxt, x0, m, mask_dx=True, **kw)
    assert (x0 == 0).any() and (x0 < 0).any()
    assert torch.equal(masked[0], torch.where(x0 > 0, plain[0], torch.zeros_like(plain[0])))
    assert len(masked) == len(plain)
    for a, b in zip(masked[1:], plain[1:]):   # dmask_part (and prev_part): unchanged
        assert torch.equal(a, b)


def _bnin_inputs(shape):
    B, C, T, V = shape
    dy, y, s, inp = _t(shape, 11), _act(shape, 12), _t(shape, 13), _act(shape, 14)
    coef = _t((3, C), 15)
    xpos = _t((C,), 16, 1e-8)
    ypos = _t((C,), 17, 2.0)
    ypos[C - 1] = 5.5      # |ypos| > 4: leaves the padded plane (range-checked loop)
    return dy, y, s, coef, inp, xpos, ypos


@pytest.mark.parametrize("shape", RA_SHAPES)
def test_tshift_bwd_bnin_premasked(shape):
    from shiftgcn import ops
    dy, y, s, coef, inp, xpos, ypos = _bnin_inputs(shape)
    ref = ops.tshift_bwd_bnin(dy, y, s, coef, inp, xpos, ypos)
    pre = torch.where(y > 0, dy, torch.zeros_like(dy))
    got = ops.tshift_bwd_bnin(pre, None, s, coef, inp, xpos, ypos)
    for a, b, n in zip(got, ref, ("gin", "gx", "gy")):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("res", [False, True])
def test_bn_bwd_premasked(shape, res):
    from shiftgcn import ops
    B, C, T, V = shape
    dy, y, x, st = _t(shape, 21), _act(shape, 22), _t(shape, 23), _stats(C, 24)
    r, rst = (_t(shape, 25), _stats(C, 26)) if res else (None, None)
    pre = torch.where(y > 0, dy, torch.zeros_like(dy))
    ref = ops.bn_bwd_reduce(dy, y, True, x, st, False, r=r, rst=rst)
    got = ops.bn_bwd_reduce(pre, None, False, x, st, False, r=r, rst=rst)
    assert torch.equal(got[0], ref[0])
    assert (got[1] is None and ref[1] is None) or torch.equal(got[1], ref[1])
    coef, rcoef = _t((3, C), 27), (_t((3, C), 28) if res else None)
    outs = []
    for d, yy, relu in ((dy, y, True), (pre, None, False)):
        dr = torch.empty_like(x)
        dx = ops.bn_bwd_apply(d, yy, relu, x, coef, False, r=r, rcoef=rcoef, dr=dr)
        outs.append((dx, dr))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("shape", SHAPES)
def test_bn_bwd_reduce_plane_dy(shape):
    from shiftgcn import ops
    B, C, T, V = shape
    dyp, y, x, st = _t((B, C), 31), _act(shape, 32), _t(shape, 33), _stats(C, 34)
    full = _expand(dyp, shape)
    for yy, relu in ((y, True), (None, False)):
        ref = ops.bn_bwd_reduce(full, yy, relu, x, st, False)
        got = ops.bn_bwd_reduce(dyp, yy, relu, x, st, False)
        assert torch.equal(got[0], ref[0])
    r, rst = _t(shape, 35), _stats(C, 36)
    ref = ops.bn_bwd_reduce(full, y, True, x, st, False, r=r, rst=rst)
    got = ops.bn_bwd_reduce(dyp, y, True, x, st, False, r=r, rst=rst)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("shape", RA_SHAPES)
def test_tshift_bwd_bnin_plane_dy(shape):
    from shiftgcn import ops
    B, C = shape[:2]
    _, y, s, coef, inp, xpos, ypos = _bnin_inputs(shape)
    dyp = _t((B, C), 41)
    full = _expand(dyp, shape)
    for yy in (y, None):
        ref = ops.tshift_bwd_bnin(full, yy, s, coef, inp, xpos, ypos)
        got = ops.tshift_bwd_bnin(dyp, yy, s, coef, inp, xpos, ypos)
        for a, b, n in zip(got, ref, ("gin", "gx", "gy")):
            assert torch.equal(a, b), n


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prev", [False, True])
def test_dx_finish_plane_add2(shape, prev):
    from shiftgcn import ops
    B, C, T, V = shape
    dxt, x0, m = _t(shape, 51), _act(shape, 52), _t((V, C), 53) + 1.0
    add1, a2m, a2p = _t(shape, 54), _act(shape, 55), _t((B, C), 56)
    kw = {"prev": (_t(shape, 57), _stats(C, 58))} if prev else {}
    ref = ops.gcn_dx_finish(dxt, x0, m, add1=add1, add2=_expand(a2p, shape), add2_mask=a2m, **kw)
    got = ops.gcn_dx_finish(dxt, x0, m, add1=add1, add2=a2p, add2_mask=a2m, **kw)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,M,C,T,V", [(2, 2, 5, 7, 25), (3, 1, 4, 5, 33)])
def test_pool_bwd_planes(N, M, C, T, V):
    from shiftgcn import ops
    dout = _t((N, C), 61)
    shape = (N * M, C, T, V)
    full = ops.pool_bwd(dout, shape, N, M)
    planes = ops.pool_bwd(dout, shape, N, M, planes=True)
    assert planes.shape == (N * M, C)
    assert torch.equal(planes, full[:, :, 0, 0])
    assert torch.equal(_expand(planes, shape), full)


# --------------------------------------------------------------------------------------
# chain and model level: the knob on against the knob off, bit for bit
# --------------------------------------------------------------------------------------
def _grads(module, x, run):
    """Every parameter gradient and the input gradient of one backward of ``run(x)``."""
    module.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    run(xr).backward()
    torch.cuda.synchronize()
    g = {n: p.grad.clone() for n, p in module.named_parameters() if p.grad is not None}
    g["input"] = xr.grad.clone()
    return g


def _ab(module, x, run, monkeypatch):
    from shiftgcn import fused
    monkeypatch.setattr(fused, "PREMASK", 0)
    ref = _grads(module, x, run)
    monkeypatch.setattr(fused, "PREMASK", 1)
    got = _grads(module, x, run)
    assert ref.keys() == got.keys() and len(ref) > 1
    for n in ref:
        assert torch.equal(got[n], ref[n]), n
    return ref


def _chain(layout, seed):
    import shiftgcn
    units = torch.nn.ModuleList(
        [shiftgcn.TCN_GCN_unit(ci, co, None, stride=s, num_point=25) for ci, co, s in layout])
    formula.fill_state(units, seed=seed)
    return units.to(DEV).train()


def _run_chain(units, weight):
    import shiftgcn

    def run(x):
        with shiftgcn.shift_gcn.linked_units(list(units)):
            for u in units:
                x = u(x)
        return (x * weight).sum()
    return run


@pytest.mark.parametrize("layout", [
    [(8, 8, 1)] * 3,
    [(8, 8, 1), (8, 16, 2), (16, 16, 1), (16, 16, 1)],
], ids=["iii", "i_down_ii"])
def test_chain_bit_identical(layout, monkeypatch):
    units = _chain(layout, 7)
    T = 8
    for _, _, s in layout:
        T //= s
    x = _t((2, 8, 8, 25), 71)
    w = _t((2, layout[-1][1], T, 25), 72)
    _ab(units, x, _run_chain(units, w), monkeypatch)


def test_chain_marks_gradients(monkeypatch):
    """identity -> (8->16, stride 2) -> identity -> identity: the third unit masks for the
    second (which has a residual conv: its own bn2 partials are not made by the third), the
    fourth for the third; the second cannot mask for the first."""
    from shiftgcn import fused
    units = _chain([(8, 8, 1), (8, 16, 2), (16, 16, 1), (16, 16, 1)], 9)
    seen = []
    real = fused._unit_backward

    def spy(unit, s, dout, off):
        seen.append((list(units).index(unit), fused.premasked(s, dout)))
        return real(unit, s, dout, off)

    monkeypatch.setattr(fused, "_unit_backward", spy)
    monkeypatch.setattr(fused, "PREMASK", 1)
    _grads(units, _t((2, 8, 8, 25), 73), _run_chain(units, _t((2, 16, 4, 25), 74)))
    assert sorted(seen) == [(0, False), (1, True), (2, True), (3, False)]


@pytest.mark.parametrize("async_dw", [0, 1])
def test_model_bit_identical_and_paths(async_dw, monkeypatch):
    import shiftgcn
    from shiftgcn import fused, ops
    monkeypatch.setattr(fused, "ASYNC_DW", async_dw)
    m = shiftgcn.Model(num_class=60, num_point=25, num_person=2,
                       graph="graph.ntu_rgb_d.Graph").to(DEV).train()
    formula.fill_state(m, seed=5)
    x = formula.tensor((2, 3, 16, 25, 2), 5, 1.0).to(DEV)
    w = _t((2, 60), 81)
    _ab(m, x, lambda xr: (m(xr) * w).sum(), monkeypatch)
    # paths taken with the knob on: no full-tensor pool gradient; l1, l2, l3, l5, l6, l8, l9
    # receive a marked (pre-masked) gradient, l10 a per-plane one
    calls = {"pool_bwd": 0}
    real_pool, real_bwd = ops.pool_bwd, fused._unit_backward
    units = [getattr(m, f"l{k}") for k in range(1, 11)]
    marked, plane = [], []

    def pool_bwd(*a, planes=False, **k):
        calls["pool_bwd"] += not planes      # the full-tensor form
        return real_pool(*a, planes=planes, **k)

    def spy(unit, s, dout, off):
        k = units.index(unit) + 1
        if fused.premasked(s, dout):
            marked.append(k)
        if dout.dim() == 2:
            plane.append(k)
        return real_bwd(unit, s, dout, off)

    monkeypatch.setattr(ops, "pool_bwd", pool_bwd)
    monkeypatch.setattr(fused, "_unit_backward", spy)
    monkeypatch.setattr(fused, "PREMASK", 1)
    _grads(m, x, lambda xr: (m(xr) * w).sum())
    assert calls["pool_bwd"] == 0
    assert sorted(marked) == [1, 2, 3, 5, 6, 8, 9]
    assert plane == [10]


def test_hook_sees_unmasked_gradient(monkeypatch):
    """A tensor hook on an intermediate output must see the gradient autograd defines (not
    the masked one), and every gradient stays what it is without the hook."""
    from shiftgcn import fused
    units = _chain([(8, 8, 1)] * 3, 11)
    x, w = _t((2, 8, 8, 25), 91), _t((2, 8, 8, 25), 92)
    run = _run_chain(units, w)
    monkeypatch.setattr(fused, "PREMASK", 0)
    ref = _grads(units, x, run)
    seen = {}

    def fwd_hook(mod, inp, out):
        seen["out"] = out.detach()
        out.register_hook(lambda g: seen.__setitem__("grad", g.clone()))

    outs = {}
    for knob in (0, 1):
        monkeypatch.setattr(fused, "PREMASK", knob)
        h = units[1].register_forward_hook(fwd_hook)
        try:
            got = _grads(units, x, run)
        finally:
            h.remove()
        outs[knob] = seen.pop("grad")
        for n in ref:
            assert torch.equal(got[n], ref[n]), (knob, n)
    assert torch.equal(outs[1], outs[0])
    # the unmasked gradient is non-zero somewhere the output is not positive
    assert (outs[1][seen["out"] <= 0] != 0).any()


def test_unit_expanded_gradient_takes_planes(monkeypatch):
    """``unit(x).mean().backward()`` and ``unit(x).sum().backward()`` against the same
    gradient materialised. sum's backward hands the unit an expanded gradient (strides 0 over
    (T, V)), which is taken per plane; mean's backward divides after expanding, so torch
    hands over a dense tensor and the unit takes the ordinary path (equal either way)."""
    from shiftgcn import fused
    units = _chain([(8, 8, 1)], 13)
    unit = units[0]
    x = _t((2, 8, 8, 25), 95)
    n = 2 * 8 * 8 * 25
    monkeypatch.setattr(fused, "PREMASK", 1)
    planes = []
    real = fused._unit_backward

    def spy(u, s, dout, off):
        planes.append(dout.dim() == 2)
        return real(u, s, dout, off)

    monkeypatch.setattr(fused, "_unit_backward", spy)
    ones = torch.ones((2, 8, 8, 25), device=DEV)
    w = ones / n    # (the same fp32 division mean's backward makes)
    for dense, expanded, plane in ((lambda y: (y * w).sum(), lambda y: y.mean(), False),
                                   (lambda y: (y * ones).sum(), lambda y: y.sum(), True)):
        del planes[:]
        ref = _grads(unit, x, lambda xr: dense(unit(xr)))
        got = _grads(unit, x, lambda xr: expanded(unit(xr)))
        assert planes == [False, plane]
        for k in ref:
            assert torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize("mode", ["retain_grad", "autograd_grad"])
def test_retained_and_captured_gradients_unmasked(mode, monkeypatch):
    """``retain_grad`` on an intermediate output, and ``torch.autograd.grad`` returning it,
    see the gradient autograd defines with the knob on (equal to the knob off)."""
    import shiftgcn
    from shiftgcn import fused
    units = _chain([(8, 8, 1)] * 3, 15)
    x, w = _t((2, 8, 8, 25), 97), _t((2, 8, 8, 25), 98)

    def run(knob):
        monkeypatch.setattr(fused, "PREMASK", knob)
        units.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        with shiftgcn.shift_gcn.linked_units(list(units)):
            a = units[0](xr)
            b = units[1](a)
            c = units[2](b)
        loss = (c * w).sum()
        if mode == "retain_grad":
            b.retain_grad()
            loss.backward()
            out = [b.grad.clone(), xr.grad.clone()]
        else:
            out = [g.clone() for g in torch.autograd.grad(loss, [b, xr])]
        torch.cuda.synchronize()
        return out + [b.detach()]

    ref, got = run(0), run(1)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert (got[0][got[2] <= 0] != 0).any()     # not the masked gradient
