"""Pin the float64 restatements of the head, pooling, finalize, SGD and modality kernels
(oracle/head_ref.py) without a GPU: against nn.BatchNorm1d in double with the permutes of
Model.forward (shift_gcn.py:194-198), forward and autograd, in train and eval mode; against
the pooling expression and its autograd; against torch.optim.SGD on double tensors; against
oracle.ensemble_oracle.derive_modalities for the two real bone tables. Check that the tables
of tests/test_gpu_head_ref.py (oracle/head_cases.py) reach every class a launch can reach,
that their gradient seeds leave no column sum near zero, and that the SUM bar is fair to
sgcn_head_moments on the table's inputs: a float32 emulation of the kernel's arithmetic holds
it with room. The same emulation with the first-frame pivot the kernel had misses it on the
two conditioning columns at T = 300 by 10 to 30 times, with the column-mean pivot it holds it.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import ensemble_oracle as eo
from oracle import head_cases as hc
from oracle import head_ref as hr
from oracle import stream_cases as sc
from oracle import stream_ref as sr

F64 = torch.float64
TOL = 1e-12
SUM = 1e-5        # tests/test_gpu_stream_ref.py's bar for sums


def _t(shape, seed, scale=1.0, offset=0.0):
    return sc.t(shape, seed, scale, offset).double()


def _close(a, b, tol=TOL):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) <= tol * (float(b.abs().max()) + 1e-300)


# --------------------------------------------------------------------------------------
# head + finalizes against nn.BatchNorm1d
# --------------------------------------------------------------------------------------
def _data_bn(F, seed):
    bn = nn.BatchNorm1d(F).double()
    with torch.no_grad():
        bn.weight.copy_(_t((F,), seed, 0.4, 1.0))
        bn.bias.copy_(_t((F,), seed + 1, 0.3))
        bn.running_mean.copy_(_t((F,), seed + 2, 0.2))
        bn.running_var.copy_(_t((F,), seed + 3, 0.3, 1.0))
    return bn


def _model_head(bn, x):
    """Model.forward's input side (shift_gcn.py:194-198)."""
    N, C, T, V, M = x.shape
    y = x.permute(0, 4, 3, 1, 2).contiguous().view(N, M * V * C, T)
    y = bn(y)
    return y.view(N, M, V, C, T).permute(0, 1, 3, 4, 2).contiguous().view(N * M, C, T, V)


@pytest.mark.parametrize("clip", [(3, 3, 7, 5, 2), (2, 2, 4, 3, 3), (1, 1, 6, 4, 1)])
@pytest.mark.parametrize("momentum", [0.1, 1.0])
def test_head_train_mode(clip, momentum):
    N, C, T, V, M = clip
    F = M * V * C
    bn = _data_bn(F, 10)
    bn.momentum = momentum
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    x = _t(clip, 1, 2.0, 0.3).requires_grad_(True)
    g = _t((N * M, C, T, V), 2)
    y = _model_head(bn.train(), x)
    y.backward(g)
    part = hr.head_moments(x)
    mean, invstd, scale, shift, rm, rv, n = hr.bn_finalize(
        part, N, T, bn.weight, bn.bias, bn.eps, momentum, rm0, rv0, 0)
    assert n == N * T and int(bn.num_batches_tracked) == 1
    assert _close(hr.head_apply(x, scale, shift), y)
    assert _close(rm, bn.running_mean) and _close(rv, bn.running_var)
    bpart = hr.head_bwd_reduce(g, x, mean, invstd)
    dg, db, coef = hr.bn_bwd_finalize(bpart, N * T, 0, mean, invstd, bn.weight)
    assert _close(dg, bn.weight.grad, 1e-11) and _close(db, bn.bias.grad, 1e-11)
    assert _close(hr.head_bwd_apply(g, x, coef), x.grad, 1e-10)
    # accumulate: added to what the gradients held; no gamma / beta: an affine-free BatchNorm
    dg2, db2, _ = hr.bn_bwd_finalize(bpart, N * T, 0, mean, invstd, bn.weight, (dg, db))
    assert _close(dg2, 2 * dg) and _close(db2, 2 * db)
    plain = nn.BatchNorm1d(F, affine=False, track_running_stats=False).double()
    m_, i_, sc_, sh_, rm_, rv_, _ = hr.bn_finalize(part, N, T, None, None, plain.eps, 0.1, None,
                                                  None, 0)
    assert rm_ is None and rv_ is None
    assert _close(hr.head_apply(x, sc_, sh_), _model_head(plain, x.detach()))


@pytest.mark.parametrize("clip", [(3, 3, 7, 5, 2), (1, 2, 5, 4, 3)])
def test_head_eval_mode(clip):
    N, C, T, V, M = clip
    F = M * V * C
    bn = _data_bn(F, 20).eval()
    x = _t(clip, 3, 2.0, 0.3).requires_grad_(True)
    g = _t((N * M, C, T, V), 4)
    y = _model_head(bn, x)
    y.backward(g)
    mean, invstd, scale, shift = sr.bn_eval_coef(bn.weight, bn.bias, bn.running_mean,
                                                 bn.running_var, bn.eps)
    assert _close(hr.head_apply(x, scale, shift), y)
    bpart = hr.head_bwd_reduce(g, x, mean, invstd)
    dg, db, coef = hr.bn_bwd_finalize(bpart, N * T, 0, mean, invstd, bn.weight,
                                      batch_stats=False)
    assert bool((coef[1] == 0).all() and (coef[2] == 0).all())
    assert _close(dg, bn.weight.grad, 1e-11) and _close(db, bn.bias.grad, 1e-11)
    assert _close(hr.head_bwd_apply(g, x, coef), x.grad, 1e-11)


@pytest.mark.parametrize("shape", [(3, 4, 6, 5), (2, 2, 3, 33)])
def test_finalize_per_joint_mapping(shape):
    """perm_V = V: Shift_gcn.bn = BatchNorm1d(V*C) on (n*t, v*C + c) (shift_gcn.py:135-137),
    partials and statistics in the local order c*V + v."""
    B, C, T, V = shape
    bn = _data_bn(V * C, 30).train()
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    z = _t(shape, 5, 2.0, 0.3).requires_grad_(True)
    g = _t(shape, 6)
    y = bn(z.permute(0, 2, 3, 1).reshape(B * T, V * C)).view(B, T, V, C).permute(0, 3, 1, 2)
    y.backward(g)
    part = sr.moments(sr.prerotated(z.detach()), 3).reshape(B, C * V, 2)
    mean, invstd, scale, shift, rm, rv, n = hr.bn_finalize(
        part, B, T, bn.weight, bn.bias, bn.eps, bn.momentum, rm0, rv0, V)
    zd = z.detach()
    assert _close(zd * scale.view(1, C, 1, V) + shift.view(1, C, 1, V), y)
    assert _close(rm, bn.running_mean) and _close(rv, bn.running_var)
    xhat = (zd - mean.view(1, C, 1, V)) * invstd.view(1, C, 1, V)
    bpart = torch.stack((g.sum(2), (g * xhat).sum(2)), -1).reshape(B, C * V, 2)
    dg, db, coef = hr.bn_bwd_finalize(bpart, B * T, V, mean, invstd, bn.weight)
    assert _close(dg, bn.weight.grad, 1e-11) and _close(db, bn.bias.grad, 1e-11)
    k = coef.view(3, 1, C, 1, V)
    assert _close(k[0] * g + k[1] * zd + k[2], z.grad, 1e-10)
    # the two orders are inverse permutations, and not the identity
    v = torch.arange(C * V)
    assert torch.equal(hr.to_ref(hr.to_local(v, V), V), v)
    assert not torch.equal(hr.to_local(v, V), v)


def test_finalize_single_element():
    """B = 1, n_part = 1: the unbiased variance of one element is its biased one (0)."""
    part = torch.tensor([[[2.5, 0.0], [-1.0, 0.0]]], dtype=F64)
    rm0, rv0 = torch.tensor([1.0, 2.0], dtype=F64), torch.tensor([3.0, 4.0], dtype=F64)
    mean, invstd, scale, shift, rm, rv, n = hr.bn_finalize(part, 1, 1, None, None, 1e-5, 0.1,
                                                           rm0, rv0, 0)
    assert n == 1 and _close(mean, part[0, :, 0])
    assert _close(invstd, torch.full((2,), 1e-5, dtype=F64).rsqrt())
    assert _close(rm, 0.9 * rm0 + 0.1 * mean) and _close(rv, 0.9 * rv0)


# --------------------------------------------------------------------------------------
# pooling
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 2, 3, 7), (1, 3, 2, 5), (3, 1, 4, 1)])
def test_pool(case):
    N, M, C, P = case
    x = _t((N * M, C, P), 7).requires_grad_(True)
    out = x.view(N, M, C, -1).mean(3).mean(1)
    dout = _t((N, C), 8)
    out.backward(dout)
    assert _close(hr.pool(x, N, M), out)
    assert _close(hr.pool_bwd(dout, M, P), x.grad)
    assert _close(hr.pool_bwd_planes(dout, M, P), x.grad[:, :, 0])
    f32 = hr.pool_bwd_f32(dout.float(), M, P)
    assert f32.dtype == np.float32 and f32.shape == (N * M, C, P)
    assert np.abs(f32 - x.grad.numpy()).max() <= 2e-7 * float(x.grad.abs().max())
    assert np.array_equal(f32[:, :, 0], hr.pool_bwd_planes_f32(dout.float(), M, P))


# --------------------------------------------------------------------------------------
# SGD
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_sgd_step(momentum, nesterov, wd):
    lr = 0.1
    p = nn.Parameter(_t((37,), 9))
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=wd)
    mine, buf = p.detach().clone(), None
    for step in range(3):
        g = _t((37,), 10 + step)
        p.grad = g.clone()
        opt.step()
        mine, buf, gs = hr.sgd_step(mine, g, buf, wd, lr, momentum, nesterov, step == 0)
        assert _close(mine, p) and torch.equal(gs, g)
        if momentum:
            assert _close(buf, opt.state[p]["momentum_buffer"])
        else:
            assert buf is None
    # the gradient scale is applied first and returned
    a = hr.sgd_step(mine, g, buf, wd, lr, momentum, nesterov, False, scale=0.25)
    b = hr.sgd_step(mine, g * 0.25, buf, wd, lr, momentum, nesterov, False)
    assert _close(a[0], b[0]) and _close(a[2], g * 0.25)


# --------------------------------------------------------------------------------------
# modalities
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,M", [(25, 2), (33, 1)])
def test_modalities(V, M):
    from shiftgcn import ensemble as ens
    pairs = ens.NTU_BONE_PAIRS if V == 25 else ens.MEDIAPIPE_BONE_PAIRS
    parent = ens.parent_table(pairs, V)
    N, C, T = 2, 3, 5
    joint = sc.t((N, C, T, V, M), 11)
    ref = eo.derive_modalities(joint.numpy(), pairs)
    f32 = hr.modalities_f32(joint, parent)
    f64 = hr.modalities(joint, parent)
    f32p = hr.modalities_f32(joint, parent, planes=True)
    scale, shift = _t((4, M * V * C), 12, 0.5, 1.0), _t((4, M * V * C), 13)
    aff = hr.modalities(joint, parent, scale, shift, planes=True)
    for k, s in enumerate(eo.MODALITIES):
        assert np.array_equal(f32[k].numpy(), ref[s]), s
        assert float((f64[k] - torch.from_numpy(ref[s]).double()).abs().max()) <= 3e-7, s
        planes = ref[s].transpose(0, 4, 1, 2, 3).reshape(N * M, C, T, V)
        assert np.array_equal(f32p[k].numpy(), planes), s
        # with the affine: data_bn in eval mode on the permuted stream (shift_gcn.py:194-198)
        x = f64[k].permute(0, 4, 3, 1, 2).reshape(N, M * V * C, T)
        x = x * scale[k][None, :, None] + shift[k][None, :, None]
        x = x.view(N, M, V, C, T).permute(0, 1, 3, 4, 2).reshape(N * M, C, T, V)
        assert _close(aff[k], x), s


def test_synthetic_parent():
    for V, _ in hc.MOD_VM:
        par = hc.synthetic_parent(V)
        v = np.arange(V)
        assert par.dtype == np.int32 and par.min() >= 0 and par.max() < V
        assert int((par == v).sum()) >= 3 and int((par > v).sum()) >= 2 and (par < v).any()
        # a transposed or dropped lookup is visible: parent[v] != v on most joints
        assert int((par != v).sum()) >= V - 4
    for C in hc.MOD_C:          # totals that are no multiple of the 256-thread workgroup
        for T in hc.MOD_T:
            for V, M in hc.MOD_VM:
                assert (hc.MOD_N * M * C * T * V) % 256


# --------------------------------------------------------------------------------------
# coverage of the tables
# --------------------------------------------------------------------------------------
def test_head_table_covers_every_class():
    have = set()
    for N, C, T, V, M in hc.HEAD_CLIPS:
        assert N * C * T * V * M <= 200_000
        G = hc.head_form(V, M)[1]
        have |= {(hc.j_class(V, M), tc) for tc in hc.t_classes(T, G)}
    reach = hc.reachable_head_classes()
    assert {j for j, _ in reach} == {"div", "idle", "idle1", "full", "ragged", "tiles"}
    assert reach <= have, sorted(reach - have)
    clips = hc.HEAD_CLIPS + hc.COND_CLIPS
    assert {c[1] for c in clips} == {1, 2, 3} and {c[0] for c in hc.HEAD_CLIPS} == {1, 3}
    assert {c[4] for c in clips} == {1, 2, 3}
    # the column counts the kernels' comments single out
    assert {c[3] * c[4] for c in hc.HEAD_CLIPS} >= {1, 2, 32, 64, 50, 33, 75, 256, 300, 512}
    assert hc.head_form(25, 2) == (50, 5, 1) and hc.head_form(100, 3) == (256, 1, 2)
    for c in hc.COND_CLIPS:
        assert c[2] in (300, 64) and np.prod(c) <= 200_000
    assert {hc.head_form(c[3], c[4])[1] > 1 for c in hc.COND_CLIPS} == {True, False}


def test_pool_table_covers_every_class():
    have = {hc.pool_class(c[3]) for c in hc.POOL_CASES}
    reach = {hc.pool_class(P) for P in range(1, 4 * 1024 + 2)}
    # the loop carries no state but its sums, so how many full trips run and how the last one
    # meets the end of the plane are independent: each is covered on its own
    for k in (0, 1):
        assert {c[k] for c in reach} == {c[k] for c in have}
    assert {(0, "lt256"), (0, "eq256"), (0, "gt256"), (1, "none"), (1, "lt256"),
            (2, "lt256")} <= have
    assert {hc.pool_bwd_class(*c) for c in hc.POOL_CASES} == {
        ("tail", "straddle"), ("whole", "straddle"), ("whole", "rows")}
    assert hc.pool_bwd_class(1, 1, 3, 5)[0] == "tail" and hc.pool_bwd_class(2, 2, 3, 7) == (
        "whole", "straddle")
    assert {c[1] for c in hc.POOL_CASES} == {1, 2, 3}
    assert any(c[3] == 1 for c in hc.POOL_CASES)


def test_finalize_table_covers_every_class():
    have = set().union(*(hc.fin_classes(B) for B in hc.FIN_B))
    reach = set().union(*(hc.fin_classes(B) for B in range(1, 66)))
    assert reach <= have, sorted(reach - have)
    assert set(hc.FIN_B) >= {1, 2, 7, 8, 9, 24, 25, 32, 33, 40, 64, 65}
    # the unroll bound b + 24 < B: B = 24 leaves wave 0 three remainder rows, B = 25 gives it
    # one unrolled trip; B = 32 / 33 likewise for wave 7 / the first remainder after a trip
    assert hc.fin_wave_rows(24, 0) == (0, 3) and hc.fin_wave_rows(25, 0) == (1, 0)
    assert hc.fin_wave_rows(32, 7) == (1, 0) and hc.fin_wave_rows(33, 0) == (1, 1)
    assert hc.fin_wave_rows(65, 0) == (2, 1) and hc.fin_wave_rows(1, 1) == (0, 0)
    for B in range(1, 80):      # every row is taken once
        assert sum(4 * t + r for t, r in (hc.fin_wave_rows(B, w) for w in range(8))) == B
    assert {hc.fin_f_class(F) for F in hc.FIN_F} == {hc.fin_f_class(F) for F in range(1, 2000)}
    assert hc.fin_perm_Vs(1600) == [0, 25] and hc.fin_perm_Vs(66) == [0, 33]
    assert max(hc.FIN_B) * max(hc.FIN_F) <= 65 * 1600


def test_sgd_table():
    offs, size = hc.sgd_layout()
    assert sorted(hc.SGD_NUMEL) == [1, 255, 256, 257, 2047, 2048, 2049, 4097, 5000]
    used = np.zeros(size, dtype=int)
    for o, n in zip(offs, hc.SGD_NUMEL):
        assert o % 2 == 1
        used[o:o + n] += 1
    assert used.max() == 1 and not used[0] and not used[-1]
    gaps = np.diff(np.flatnonzero(np.diff(used) != 0))[1::2]     # runs of sentinel between
    assert gaps.min() >= 1 and gaps.max() <= 3 and len(set(gaps)) == 3
    ch = hc.sgd_chunks()
    assert sorted(ch) != ch and len(set(ch)) == len(ch)
    for t, n in enumerate(hc.SGD_NUMEL):     # every element in exactly one chunk
        assert sorted(s for tt, s in ch if tt == t) == list(range(0, n, hc.SGD_CHUNK))
    # chunk edges and thread-stride edges: a last chunk of 1, 2047 and 2048 elements
    tails = {n - s for t, n in enumerate(hc.SGD_NUMEL) for s in range(0, n, hc.SGD_CHUNK)}
    assert {1, 255, 256, 257, 2047, 2048} <= tails
    tab = hc.sgd_table([(8, 16, 24)], [(0.5, 0.25)], [3], [0.125])
    assert tab.dtype == np.int64 and tab.shape == (1, 5)
    assert tab[0, 3] == 0x3F000000 | 0x3E800000 << 32 and tab[0, 4] == 3 | 0x3E000000 << 32
    assert hc.sgd_table([(8, 16, 24)], [4096], [4], [0.0])[0, 3:].tolist() == [4096, 4]


# --------------------------------------------------------------------------------------
# conditioning
# --------------------------------------------------------------------------------------
def _rel(got, ref):
    """per kind of sum: max |got - ref| / max |ref|, as the GPU test's _check_sums"""
    got = torch.as_tensor(got).double()
    return [float((got[..., j] - ref[..., j]).abs().max()) /
            (float(ref[..., j].abs().max()) + 1e-300) for j in range(ref.shape[-1])]


def test_gradient_seeds_leave_no_column_near_zero():
    """sgcn_head_bwd_reduce's sums are compared with the largest sum of their kind: that one
    must not be a cancelled sum (the streaming suite's lesson)."""
    worst = 0.0
    for clip in hc.HEAD_CLIPS:
        N, C, T, V, M = clip
        k = hc.head_inputs(clip)
        gf = hr._feat_planes(k["g"], N, M)
        xhat = (hr._feat(k["x"]) - hr._fvec(k["mean"], k["x"])) * hr._fvec(k["invstd"], k["x"])
        ref = hr.head_bwd_reduce(k["g"], k["x"], k["mean"], k["invstd"])
        for j, terms in enumerate((gf, gf * xhat)):
            cond = float(terms.abs().sum(-1).max()) / float(ref[..., j].abs().max())
            worst = max(worst, cond)
            assert cond <= 8.0, (clip, j, cond)
    print(f"head_bwd_reduce: worst sum |terms| / max |sum| = {worst:.2f}")


def test_sum_bar_is_fair_to_head_moments():
    """The float32 arithmetic of head_moments_kernel, emulated, holds SUM on every clip of the
    table with room (a quarter of the bar), with any pivot: the bar asks nothing a correct
    float32 kernel cannot give. The table's columns are uniform noise, the first frame within
    sqrt(3) deviations of the mean: the kernel keeps its first-frame sums on all of them."""
    worst = {"first": 0.0, "mean": 0.0, "kernel": 0.0}
    for clip in hc.HEAD_CLIPS:
        x = hc.head_inputs(clip)["x"]
        ref = hr.head_moments(x)
        for pivot in worst:
            for r in _rel(hc.emulate_head_moments(x.numpy(), pivot), ref):
                worst[pivot] = max(worst[pivot], r)
                assert r <= SUM / 4, (clip, pivot, r)
        assert not hc.emulate_head_moments(x.numpy(), "kernel", with_again=True)[1].any()
    print("head_moments emulation, table inputs: worst share of SUM "
          + ", ".join(f"{p} pivot {v / SUM:.3f}" for p, v in worst.items()))


@pytest.mark.parametrize("clip", hc.COND_EDGE_CLIPS, ids=lambda c: "x".join(map(str, c)))
def test_conditioning_columns_by_emulation(clip):
    """What the emulation gives on the adversarial columns. (a), (b): the first-frame pivot
    alone misses SUM on M2 (the finding, recorded without a GPU; the shortest clips of the
    table, T = 64, show it least), the column-mean pivot holds it, and the kernel takes the
    column-mean pivot on every such column. (c): the first frame sits where the kernel decides;
    both decisions occur, and the first-frame sums it keeps hold SUM."""
    for kind in ("a", "b") if clip in hc.COND_CLIPS else ():
        x = hc.cond_clip(clip, kind)
        ref = hr.head_moments(x)
        first = _rel(hc.emulate_head_moments(x.numpy(), "first"), ref)
        mean = _rel(hc.emulate_head_moments(x.numpy(), "mean"), ref)
        kern, again = hc.emulate_head_moments(x.numpy(), "kernel", with_again=True)
        print(f"clip {clip} column ({kind}): M2 error / max M2: first-frame pivot "
              f"{first[1]:.2e} ({first[1] / SUM:.1f} x SUM), mean pivot {mean[1]:.2e}; "
              f"mean error: {first[0]:.2e} / {mean[0]:.2e}")
        assert max(mean) <= SUM / 4, (kind, mean)
        assert again.all() and np.array_equal(kern, hc.emulate_head_moments(x.numpy(), "mean"))
        assert first[0] <= SUM
        if clip[2] == 300:
            assert first[1] > 5 * SUM, (kind, first)
    x = hc.cond_clip(clip, "c")
    ref = hr.head_moments(x)
    kern, again = hc.emulate_head_moments(x.numpy(), "kernel", with_again=True)
    first = _rel(hc.emulate_head_moments(x.numpy(), "first"), ref)
    got = _rel(kern, ref)
    N, C, T, V, M = clip
    print(f"clip {clip} column (c): bound on q/M2 {hc.head_cond(T, hc.head_form(V, M)[1]):.1f}, "
          f"{int(again.sum())} of {again.size} columns summed again; M2 error / max M2: "
          f"kernel {got[1]:.2e} ({got[1] / SUM:.2f} x SUM), first-frame pivot alone "
          f"{first[1]:.2e}")
    assert 0.25 <= again.mean() <= 0.75, again.mean()
    assert max(got) <= SUM, got
