"""Cross-unit fusion state travels in per-call links (fused._Link), not on the modules.

* whatever becomes of a chain's graph (full backward, dropped, a backward that stops at an
  intermediate output, a frozen prefix, an exception inside the block), no module of the
  chain keeps an attribute it did not have before;
* the same chain run twice in one graph, under a block each or both inside one block, takes
  the cross-unit fusions in both calls and each call's backward uses its own forward's state;
* a unit called inside the block on a tensor that is not its predecessor's output runs
  unfused, bit for bit.
"""
import pytest
import torch

from test_gpu_premask import _chain, _run_chain, _t

pytestmark = pytest.mark.gpu

# (the smallest chains that take the linked, GBN, pre-masked and conv-residual paths)
LAYOUTS = {"iii": [(8, 8, 1)] * 3,
           "i_down_ii": [(8, 8, 1), (8, 16, 2), (16, 16, 1), (16, 16, 1)]}
X_SHAPE = (2, 8, 8, 25)
layouts = pytest.mark.parametrize("name", list(LAYOUTS))


def _out_shape(name):
    T = X_SHAPE[2]
    for _, _, s in LAYOUTS[name]:
        T //= s
    return (X_SHAPE[0], LAYOUTS[name][-1][1], T, X_SHAPE[3])


def _linked(units, x, upto=None):
    """Outputs of the chain's first ``upto`` units (all by default), linked."""
    import shiftgcn
    outs = []
    with shiftgcn.shift_gcn.linked_units(list(units)):
        for u in list(units)[:upto]:
            x = u(x)
            outs.append(x)
    return outs


def _tensors(obj, depth=6):
    """Every tensor reachable from ``obj`` through containers, __dict__ and __slots__."""
    if isinstance(obj, torch.Tensor):
        return [obj]
    if depth == 0 or obj is None or isinstance(obj, (str, bytes, int, float, torch.nn.Module)):
        return []
    if isinstance(obj, dict):
        kids = list(obj.values())
    elif isinstance(obj, (list, tuple, set, frozenset)):
        kids = list(obj)
    else:
        kids = list(getattr(obj, "__dict__", {}).values())
        for c in type(obj).__mro__:
            kids += [getattr(obj, n, None) for n in getattr(c, "__slots__", ())]
    return [t for k in kids for t in _tensors(k, depth - 1)]


def _snapshot(units):
    return {m: set(m.__dict__) for m in units.modules()}


def _assert_nothing_left(before, allow_prefix=None):
    """Every module has the attributes it had at ``before`` (plus, with ``allow_prefix``,
    the documented eval caches of ops.cached), and no new attribute holds a tensor."""
    for m, keys in before.items():
        now = set(m.__dict__)
        added = {k for k in now - keys
                 if allow_prefix is None or not k.startswith(allow_prefix)}
        held = {k: len(_tensors(m.__dict__[k])) for k in added}
        assert not any(held.values()), (type(m).__name__, "tensors held by", held)
        assert not added and keys <= now, (type(m).__name__, added, keys - now)


# --------------------------------------------------------------------------------------
# nothing is left on the modules
# --------------------------------------------------------------------------------------
def _full_backward(units, x, w):
    (_linked(units, x.requires_grad_(True))[-1] * w).sum().backward()


def _forward_only(units, x, w):
    out = _linked(units, x.requires_grad_(True))[-1]
    del out


def _grad_of_intermediate(units, x, w):
    # b = the second unit's output: the first two units' backward nodes never run
    outs = _linked(units, x.requires_grad_(True))
    torch.autograd.grad((outs[-1] * w).sum(), [outs[1]])


def _frozen_prefix(units, x, w):
    # the first unit has no backward node at all
    for p in units[0].parameters():
        p.requires_grad_(False)
    (_linked(units, x)[-1] * w).sum().backward()


def _raises_in_block(units, x, w):
    import shiftgcn
    with pytest.raises(ZeroDivisionError):
        with shiftgcn.shift_gcn.linked_units(list(units)):
            y = units[1](units[0](x.requires_grad_(True)))
            1 / 0
    y.sum().backward()


@layouts
@pytest.mark.parametrize("case", [_full_backward, _forward_only, _grad_of_intermediate,
                                  _frozen_prefix, _raises_in_block],
                         ids=lambda f: f.__name__.strip("_"))
def test_nothing_left_on_modules(name, case, monkeypatch):
    from shiftgcn import fused
    monkeypatch.setattr(fused, "PREMASK", 1)
    units = _chain(LAYOUTS[name], 21)
    before = _snapshot(units)
    case(units, _t(X_SHAPE, 101), _t(_out_shape(name), 102))
    torch.cuda.synchronize()
    _assert_nothing_left(before)


@layouts
def test_inference_leaves_only_eval_caches(name):
    units = _chain(LAYOUTS[name], 21).eval()
    before = _snapshot(units)
    with torch.no_grad():
        out = _linked(units, _t(X_SHAPE, 101))[-1]
    torch.cuda.synchronize()
    assert out.shape == _out_shape(name)
    _assert_nothing_left(before, allow_prefix="_sgcn_")


# --------------------------------------------------------------------------------------
# two calls, one graph
# --------------------------------------------------------------------------------------
def _two_call_grads(units, run, a, b, one_graph, one_block=False):
    import shiftgcn
    units.zero_grad(set_to_none=True)
    xa, xb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    if one_block:               # both calls inside ONE linked_units block, one backward
        with shiftgcn.shift_gcn.linked_units(list(units)):
            loss = run(xa, link=False) + run(xb, link=False)
        loss.backward()
    elif one_graph:
        (run(xa) + run(xb)).backward()
    else:                       # two accumulating backward passes
        run(xa).backward()
        run(xb).backward()
    torch.cuda.synchronize()
    g = {n: p.grad.clone() for n, p in units.named_parameters() if p.grad is not None}
    g["a"], g["b"] = xa.grad.clone(), xb.grad.clone()
    return g


def _two_call_setup(name, monkeypatch):
    """(chain, inputs a and b, run(x, link=True) -> loss, the list a spy on _unit_backward
    fills with (unit, its gradient arrived pre-masked))."""
    from shiftgcn import fused
    monkeypatch.setattr(fused, "PREMASK", 1)
    units = _chain(LAYOUTS[name], 23)
    w = _t(_out_shape(name), 113)

    def run(x, link=True):
        if link:
            return _run_chain(units, w)(x)
        for u in units:
            x = u(x)
        return (x * w).sum()

    seen = []
    real = fused._unit_backward

    def spy(unit, s, dout, off):
        seen.append((list(units).index(unit), fused.premasked(s, dout)))
        return real(unit, s, dout, off)

    monkeypatch.setattr(fused, "_unit_backward", spy)
    return units, _t(X_SHAPE, 111), _t(X_SHAPE, 112), run, seen


def _single_call_marks(units, run, a, seen):
    """The pre-masked set of ONE linked call's backward, as the spy records it."""
    del seen[:]
    units.zero_grad(set_to_none=True)
    run(a.clone().requires_grad_(True)).backward()
    torch.cuda.synchronize()
    single = sorted(seen)
    assert len(single) == len(units) and any(m for _, m in single)
    return single


@layouts
def test_two_calls_one_graph(name, monkeypatch):
    """The same chain under two linked_units blocks, one backward of the summed losses: the
    gradients of two accumulating passes, and both calls take the fusions (neither borrows
    the other's state): the single call's pre-masked set, twice over."""
    from shiftgcn import fused
    units, a, b, run, seen = _two_call_setup(name, monkeypatch)
    monkeypatch.setattr(fused, "ASYNC_DW", 0)
    ref = _two_call_grads(units, run, a, b, one_graph=False)
    single = _single_call_marks(units, run, a, seen)
    for async_dw in (0, 1):
        monkeypatch.setattr(fused, "ASYNC_DW", async_dw)
        del seen[:]
        got = _two_call_grads(units, run, a, b, one_graph=True)
        assert sorted(seen) == sorted(single * 2), async_dw
        assert got.keys() == ref.keys() and len(got) > 2
        for n in ref:
            torch.testing.assert_close(got[n], ref[n], rtol=1e-6, atol=1e-7, msg=n)


@layouts
def test_two_calls_one_block(name, monkeypatch):
    """The chain run twice inside ONE linked_units block (a producer is called again after
    its consumer ran): each call's backward uses what ITS forward handed over. Bit for bit
    the gradients of the two calls under a block each, with the same fusions taken."""
    from shiftgcn import fused
    units, a, b, run, seen = _two_call_setup(name, monkeypatch)
    single = _single_call_marks(units, run, a, seen)
    for async_dw in (0, 1):
        monkeypatch.setattr(fused, "ASYNC_DW", async_dw)
        ref = _two_call_grads(units, run, a, b, one_graph=True)
        del seen[:]
        got = _two_call_grads(units, run, a, b, one_graph=True, one_block=True)
        assert sorted(seen) == sorted(single * 2), async_dw
        assert got.keys() == ref.keys() and len(got) > 2
        for n in ref:
            assert torch.equal(got[n], ref[n]), (async_dw, n)


# --------------------------------------------------------------------------------------
# off-chain input
# --------------------------------------------------------------------------------------
@layouts
def test_off_chain_input_runs_unfused(name, monkeypatch):
    """The second unit is called on a clone of the first unit's output: it must not take
    what the first unit's tail launch made for that output, nor hand the first unit its
    backward partials or a masked gradient. Equal to every unit run unlinked."""
    import contextlib

    import shiftgcn
    from shiftgcn import fused
    monkeypatch.setattr(fused, "PREMASK", 1)
    units = _chain(LAYOUTS[name], 25)
    x, w = _t(X_SHAPE, 121), _t(_out_shape(name), 122)

    def grads(linked):
        units.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        block = shiftgcn.shift_gcn.linked_units(list(units)) if linked \
            else contextlib.nullcontext()
        with block:
            y = units[0](xr).clone()
            for u in list(units)[1:]:
                y = u(y)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        g = {n: p.grad.clone() for n, p in units.named_parameters() if p.grad is not None}
        g["input"] = xr.grad.clone()
        return g

    ref, got = grads(False), grads(True)
    assert got.keys() == ref.keys() and len(got) > 1
    for n in ref:
        assert torch.equal(got[n], ref[n]), n
