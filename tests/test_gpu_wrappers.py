"""The whole model under torch's own data-parallel wrappers: ``nn.DataParallel`` /
``torch.nn.parallel.replicate`` (a replica's parameters are non-leaf attributes) and
``DistributedDataParallel`` (its reducer hooks the AccumulateGrad nodes).

The yardstick everywhere is the single-device in-order path: ``fused.ASYNC_DW =
fused.BATCH_SIDE = 0`` on an unwrapped model with the same weights and input. Comparisons are
bit for bit: the wrappers add only exact operations (a one-term reduce-add, a division by
world size 1, ``a + b`` of two finished tensors), and every kernel is deterministic.
"""
import warnings

import pytest
import torch

import formula

pytestmark = pytest.mark.gpu

T = 16      # the shortest clip that survives both stride-2 units
STEPS = 2


def _model(dev):
    import shiftgcn
    m = shiftgcn.Model(num_class=10, num_point=25, num_person=2, graph="graph.ntu_rgb_d.Graph")
    formula.fill_state(m, seed=5)
    return m.to(dev).train()


def _batch(k, dev):
    x = formula.tensor((4, 3, T, 25, 2), 60 + k, 1.0).to(dev)
    return x, torch.tensor([1, 3, 5, 7], device=dev)


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().cpu().clone())
            for n, p in m.named_parameters() if p.requires_grad}


def _buffers(m):
    return {n: b.detach().cpu().clone() for n, b in m.named_buffers()}


class _InOrderKnobs:
    """The yardstick's setting: everything on the current stream, nothing batched."""

    def __enter__(self):
        from shiftgcn import fused
        self.old = (fused.ASYNC_DW, fused.BATCH_SIDE)
        fused.ASYNC_DW = fused.BATCH_SIDE = 0

    def __exit__(self, *exc):
        from shiftgcn import fused
        fused.ASYNC_DW, fused.BATCH_SIDE = self.old
        return False


@pytest.fixture(scope="module")
def yardstick():
    """STEPS consecutive unwrapped in-order steps: [(loss, grads, buffers)] on the CPU."""
    dev = torch.device("cuda:0")
    with _InOrderKnobs():
        m = _model(dev)
        res = []
        for k in range(STEPS):
            x, y = _batch(k, dev)
            m.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(m(x), y)
            loss.backward()
            torch.cuda.synchronize()
            res.append((loss.detach().cpu(), _grads(m), _buffers(m)))
    assert len(res[0][1]) > 100 and all(g is not None for g in res[0][1].values())
    return res


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    missing = [n for n, g in got.items() if g is None]
    assert not missing, f"{what}: no gradient for {len(missing)} parameters, e.g. {missing[:3]}"
    for n in want:
        assert torch.equal(got[n], want[n]), f"{what}: {n}"


def _bn_stat_names(m):
    import torch.nn as nn
    names = []
    for n, mod in m.named_modules():
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            names += [f"{n}.running_mean", f"{n}.running_var", f"{n}.num_batches_tracked"]
    return names


# --------------------------------------------------------------------------------------
# 1. one replica
# --------------------------------------------------------------------------------------
def test_one_replica_trains_every_parameter(yardstick):
    from shiftgcn import fused
    assert fused.ASYNC_DW == 1 and fused.BATCH_SIDE == 1     # the defaults stay on
    dev = torch.device("cuda:0")
    m = _model(dev)
    stats = _bn_stat_names(m)
    # data_bn and, per unit, gcn1.bn, tcn1.bn, tcn1.bn2 (+ down.1 / residual.bn where present)
    assert sum(n.startswith("l") for n in stats) == 3 * 35 and len(stats) == 3 * 36
    for k in range(STEPS):
        x, y = _batch(k, dev)
        m.zero_grad(set_to_none=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")     # e.g. ``.grad`` of a non-leaf tensor read
            replica = torch.nn.parallel.replicate(m, [dev])[0]
            assert replica._is_replica and not list(replica.parameters())
            loss = torch.nn.functional.cross_entropy(replica(x), y)
            loss.backward()
        torch.cuda.synchronize()
        want_loss, want_g, want_b = yardstick[k]
        assert torch.equal(loss.detach().cpu(), want_loss)
        _assert_same(_grads(m), want_g, f"step {k}")
        got_b = _buffers(m)      # replica 0's buffers ARE the master's tensors
        for n in stats:
            assert torch.equal(got_b[n], want_b[n]), f"step {k}: {n}"
        assert int(got_b["l5.tcn1.bn2.num_batches_tracked"]) == k + 1
    assert not fused._TASKS


# --------------------------------------------------------------------------------------
# 2. two replicas: DataParallel's rule
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_replica_rule():
    """oracle.dp_oracle's statement of the rule on two in-order unwrapped models (replica 0
    = the model itself, the other a deep copy) over the half batches: ONE global-mean loss,
    summed gradients, replica 0's running statistics."""
    from oracle.dp_oracle import dataparallel_grads
    dev = torch.device("cuda:0")
    with _InOrderKnobs():
        m = _model(dev)
        x, y = _batch(0, dev)
        loss, _, grads = dataparallel_grads(m, x, y, 2)
        torch.cuda.synchronize()
        return loss.cpu(), {n: g.cpu() for n, g in grads.items()}, _buffers(m)


def _check_two_replicas(m, loss, rule):
    from shiftgcn import fused
    from shiftgcn.dist import is_shift_position
    want_loss, want_g, want_b = rule
    torch.cuda.synchronize()
    assert torch.equal(loss.detach().cpu(), want_loss)
    got = _grads(m)
    _assert_same(got, want_g, "two replicas")       # ordinary: g0 + g1
    # positions: the SUM of two replicas' constrained gradients, each 0 for xpos and +-0.01
    # (0.0001 where the raw gradient is zero) for ypos, never their mean
    one = torch.tensor([0.01, -0.01, 0.0001])
    sums = (one[:, None] + one[None, :]).reshape(-1)
    for n, g in got.items():
        if is_shift_position(n) and n.endswith("xpos"):
            assert bool((g == 0).all()), n
        elif is_shift_position(n):
            assert bool(((g.reshape(-1, 1) - sums).abs().min(dim=1).values < 1e-7).all()), n
            assert bool((g.abs() > 0.015).any()), n
    got_b = _buffers(m)
    for n in _bn_stat_names(m):
        assert torch.equal(got_b[n], want_b[n]), n   # replica 0's
    assert not fused._TASKS


def test_two_replicas_on_one_device(two_replica_rule):
    """replicate(model, [dev, dev]) + parallel_apply: DataParallel's rule on one GPU, and two
    replica threads sharing the device's side stream (the forward's conv branches)."""
    from torch.nn.parallel import parallel_apply, replicate
    dev = torch.device("cuda:0")
    m = _model(dev)
    x, y = _batch(0, dev)
    m.zero_grad(set_to_none=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        reps = replicate(m, [dev, dev])
        outs = parallel_apply(reps, [(c,) for c in x.chunk(2)], devices=[dev, dev])
        loss = torch.nn.functional.cross_entropy(torch.cat(outs), y)
        loss.backward()
    _check_two_replicas(m, loss, two_replica_rule)


def test_two_replicas_data_parallel(two_replica_rule):
    if torch.cuda.device_count() < 2:
        pytest.skip("nn.DataParallel over two devices needs two GPUs")
    dev = torch.device("cuda:0")
    m = _model(dev)
    dp = torch.nn.DataParallel(m, device_ids=[0, 1])
    x, y = _batch(0, dev)
    m.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(dp(x), y)
    loss.backward()
    _check_two_replicas(m, loss, two_replica_rule)


# --------------------------------------------------------------------------------------
# 3. / 4. DistributedDataParallel, world 1
# --------------------------------------------------------------------------------------
def _init(backend, tmp_path):
    import torch.distributed as dist
    dist.init_process_group(backend, init_method=f"file://{tmp_path / 'store'}", rank=0,
                            world_size=1)


@pytest.mark.parametrize("bucket_view", [False, True])
@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_ddp_world1_gradients(yardstick, tmp_path, backend, bucket_view):
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from shiftgcn import fused
    assert fused.ASYNC_DW == 1 and fused.BATCH_SIDE == 1     # the side stream stays on
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _init(backend, tmp_path)
    try:
        m = _model(dev)
        ddp = DDP(m, device_ids=[0], gradient_as_bucket_view=bucket_view)
        for k in range(STEPS):
            x, y = _batch(k, dev)
            ddp.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(ddp(x), y)
            loss.backward()
            torch.cuda.synchronize()
            want_loss, want_g, want_b = yardstick[k]
            assert torch.equal(loss.detach().cpu(), want_loss)
            _assert_same(_grads(m), want_g, f"{backend} step {k}")
            got_b = _buffers(m)
            for n in _bn_stat_names(m):
                assert torch.equal(got_b[n], want_b[n]), f"step {k}: {n}"
        assert not fused._TASKS
        del ddp
    finally:
        dist.destroy_process_group()


def test_ddp_with_grad_allreduce_raises(tmp_path):
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from shiftgcn.dist import GradAllReduce
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _init("gloo", tmp_path)
    try:
        m = _model(dev)
        ddp = DDP(m, device_ids=[0])
        ar = GradAllReduce(m)
        try:
            x, _ = _batch(0, dev)
            with pytest.raises(RuntimeError, match="GradAllReduce"):
                ddp(x)
        finally:
            ar.close()
        del ddp
    finally:
        dist.destroy_process_group()


# --------------------------------------------------------------------------------------
# 5. the unwrapped path is untouched
# --------------------------------------------------------------------------------------
def test_block_params_of_an_ordinary_model():
    from shiftgcn import fused
    m = _model(torch.device("cuda:0"))
    for mod in (m.l1, m.l5, m.l8.gcn1, m.l9.tcn1, m.l8.residual):
        want = [(n, p) for n, p in mod.named_parameters() if p.requires_grad]
        got = fused.block_params(mod)
        assert [n for n, _ in got] == [n for n, _ in want]
        assert all(a is b for (_, a), (_, b) in zip(got, want))


def test_unwrapped_step_still_defers(yardstick, monkeypatch):
    from shiftgcn import fused
    assert fused.ASYNC_DW == 1 and fused.BATCH_SIDE == 1
    dev = torch.device("cuda:0")
    m = _model(dev)
    names = {id(p): n for n, p in m.named_parameters()}
    real, deferred = fused._accumulate, []

    def rec(p, g):
        deferred.append(names[id(p)])
        return real(p, g)

    monkeypatch.setattr(fused, "_accumulate", rec)
    x, y = _batch(0, dev)
    torch.nn.functional.cross_entropy(m(x), y).backward()
    torch.cuda.synchronize()
    # the side stream's weight gradients and the batched position / mask finalizes
    for n in ("l5.gcn1.Linear_weight", "l5.gcn1.down.0.weight", "l8.residual.conv.weight",
              "l9.tcn1.temporal_linear.weight", "l10.tcn1.shift_in.xpos",
              "l3.gcn1.Feature_Mask"):
        assert n in deferred, n
    # per unit 9 (Linear_weight/bias, Feature_Mask, temporal_linear weight/bias, 4 positions),
    # + down.0 weight/bias in l1, l5, l8 and residual.conv weight/bias in l5, l8 = 100; the
    # chain's first unit keeps all but its mask finalize on the current stream (TAIL_MAIN
    # bit 2): 10 fewer
    assert fused.TAIL_MAIN & 2
    assert len(deferred) == len(set(deferred)) == 90
    _assert_same(_grads(m), yardstick[0][1], "unwrapped, deferred")
    assert not fused._TASKS
