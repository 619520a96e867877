"""nn.DataParallel replicas on the host: ``fused.block_params`` finds a replica's parameters
(plain attributes, non-leaf, listed in ``_former_parameters``) under the master's names and
order, and ``fused._defer_ok`` never defers a gradient for them (nor inside a
DistributedDataParallel step). No GPU: the replica is built the way
``torch.nn.parallel.replicate`` builds one, with ``p.clone()`` standing in for Broadcast.
"""
from collections import OrderedDict

import torch

import shiftgcn
from shiftgcn import fused


def _host_replica(master):
    """``replicate`` (one replica) without a device: a copy of every submodule rewired to
    the copies, every parameter replaced by a non-leaf clone set as a plain attribute."""
    mods = list(master.modules())
    copies = {}
    for m in mods:
        r = m._replicate_for_data_parallel()
        r._former_parameters = OrderedDict()
        copies[m] = r
    clones = {}
    for m in mods:
        r = copies[m]
        for key, child in m._modules.items():
            if child is None:
                r._modules[key] = None
            else:
                setattr(r, key, copies[child])
        for key, p in m._parameters.items():
            if p is None:
                r._parameters[key] = None
                continue
            if p not in clones:
                clones[p] = p.clone()
            setattr(r, key, clones[p])
            r._former_parameters[key] = clones[p]
    return copies[master]


def _unit():
    u = shiftgcn.TCN_GCN_unit(8, 16, None, stride=2, residual=True, num_point=5)
    u.gcn1.Linear_bias.requires_grad_(False)   # a frozen parameter among the trainable ones
    return u


def test_ordinary_module_same_as_named_parameters():
    u = _unit()
    want = [(n, p) for n, p in u.named_parameters() if p.requires_grad]
    got = fused.block_params(u)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert all(a is b for (_, a), (_, b) in zip(got, want))
    assert "gcn1.Linear_bias" not in dict(got) and "gcn1.shift_in" not in dict(got)
    assert "residual.conv.weight" in dict(got) and "gcn1.down.1.bias" in dict(got)


def test_replica_names_order_and_tensors():
    u = _unit()
    r = _host_replica(u)
    assert r._is_replica and not list(r.parameters())   # what trainable() used to read
    want = [n for n, p in u.named_parameters() if p.requires_grad]
    got = fused.block_params(r)
    assert [n for n, _ in got] == want
    for n, t in got:
        owner = r
        *path, leaf = n.split(".")
        for part in path:
            owner = getattr(owner, part)
        assert getattr(owner, leaf) is t, n       # the tensor the forward reads
        assert not t.is_leaf and t.requires_grad, n
        assert torch.equal(t, dict(u.named_parameters())[n])
    # submodules too (a Shift_gcn or Shift_tcn replica called on its own)
    assert ([n for n, _ in fused.block_params(r.tcn1)] ==
            [n for n, p in u.tcn1.named_parameters() if p.requires_grad])


def test_tied_parameter_listed_once():
    u = _unit()
    u.tcn1.shift_out.xpos = u.tcn1.shift_in.xpos     # both have 16 channels
    r = _host_replica(u)
    want = [n for n, p in u.named_parameters() if p.requires_grad]
    assert [n for n, _ in fused.block_params(r)] == want
    assert "tcn1.shift_out.xpos" not in want


def test_defer_ok_false_for_replica_tensors():
    r = _host_replica(_unit())
    with torch.no_grad():   # (so that grad mode is not the reason)
        for n, t in fused.block_params(r):
            assert fused._defer_ok([t]) is False, n


def test_defer_ok_reasons_meet_in_one_predicate():
    """Inside a plain backward: a leaf parameter may be deferred; not a non-leaf one, and
    nothing while the block runs in order (the DistributedDataParallel flag)."""
    w = torch.nn.Parameter(torch.ones(3))
    nl = torch.nn.Parameter(torch.ones(3)).clone()
    seen = {}

    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            return a + b

        @staticmethod
        def backward(ctx, g):
            seen["leaf"] = fused._defer_ok([w])
            seen["non_leaf"] = fused._defer_ok([w, nl])
            fused._BWD.in_order = True
            try:
                seen["ddp"] = fused._defer_ok([w])
            finally:
                fused._BWD.in_order = False
            return g, g

    F.apply(w, nl).sum().backward()
    assert seen == {"leaf": True, "non_leaf": False, "ddp": False}
