"""The head, pooling, BatchNorm-finalize, SGD and modality kernels, each called alone, against
their float64 restatements (oracle/head_ref.py): sgcn_head_moments / _apply / _bwd_reduce /
_bwd_apply, sgcn_pool / _pool_bwd / _pool_bwd_planes, sgcn_bn_finalize, sgcn_bn_bwd_finalize,
sgcn_sgd_step and sgcn_modalities.

The tables (oracle/head_cases.py) are the smallest shapes that reach every class of the launch
arithmetic (idle row groups, ragged column tiles, the 8-row trips; the 4 x 256 pooling trips
and their vector tail; the 8-wave batch stride and its 4-row unroll; the 2,048-element SGD
chunks and 256-thread stride); tests/test_oracle_head.py checks that coverage, and pins the
restatements, without a GPU.

Every float input is a slice of NaN storage; every output sits at its exact extent between two
margins of a sentinel bit pattern, which must survive the call. Forms shiftgcn.ops does not
expose (NULL gamma / beta, NULL running statistics, accumulate = 1, NULL dgamma / dbeta, the
raw SGD table) go through the C entry points directly.

Bars (max |got - ref| <= bar * max |ref| over the output; test_gpu_stream_ref's):
  E6  = 1e-6  element-wise outputs of a handful of float32 operations, the finalizes' double
              merges rounded once;
  E5  = 1e-5  differences of products (shift = beta - mean*scale, k3 = -k1*mean(g) - k2*mean);
  SUM = 1e-5  sums (head_moments, head_bwd_reduce, pool), each kind as its own vector.
The pooling gradients and the modality streams without the affine are compared bit for bit
with their float32 expressions.

Measured on an MI355X (worst case over the tables, as a share of the bar): see DESIGN.md,
"Head, finalize and SGD reference tests".
"""
import numpy as np
import pytest
import torch

from oracle import head_cases as hc
from oracle import head_ref as hr
from oracle import stream_cases as sc
from test_gpu_stream_ref import E5, E6, SUM, _check, _check_sums
from test_gpu_tshift_ref import SENTINEL, _dev, _guard, _Guarded, _Stats

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(np.float32(1e-5))


def _id(c):
    return "x".join(map(str, c))


def _f(v):
    """a Python float at float32 precision: what a C float argument receives"""
    return float(np.float32(v))


def _lib():
    from shiftgcn import _lib as L
    return L, L.load()


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _unchanged(d, k):
    for n, v in d.items():      # no input was written
        assert torch.equal(v.cpu().view(torch.int32), k[n].view(torch.int32)), n


# --------------------------------------------------------------------------------------
# head kernels alone
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", hc.HEAD_CLIPS, ids=_id)
def test_head_kernels(clip):
    from shiftgcn import ops
    N, C, T, V, M = clip
    k = hc.head_inputs(clip)
    d = {n: _dev(v) for n, v in k.items()}
    st = _Stats(d["mean"], d["invstd"], d["scale"], d["shift"])
    with _guard("head_moments"):
        part = ops.head_moments(d["x"])
    _check_sums(part.cpu(), hr.head_moments(k["x"]), "head_moments")
    with _guard("head_apply"):
        y = ops.head_apply(d["x"], st)
    _check(y.cpu(), hr.head_apply(k["x"], k["scale"], k["shift"]), E6, "head_apply")
    with _guard("head_bwd_reduce"):
        bpart = ops.head_bwd_reduce(d["g"], d["x"], st)
    _check_sums(bpart.cpu(), hr.head_bwd_reduce(k["g"], k["x"], k["mean"], k["invstd"]),
                "head_bwd_reduce")
    with _guard("head_bwd_apply"):
        dx = ops.head_bwd_apply(d["g"], d["x"], d["coef"])
    assert dx.shape == tuple(clip)
    _check(dx.cpu(), hr.head_bwd_apply(k["g"], k["x"], k["coef"]), E6, "head_bwd_apply")
    _unchanged(d, k)


@pytest.mark.parametrize("clip,kind", [(c, k) for k in "ab" for c in hc.COND_CLIPS]
                         + [(c, "c") for c in hc.COND_EDGE_CLIPS], ids=_id)
def test_head_moments_conditioning(clip, kind):
    """Columns whose first frame is far from the rest: (a) a joint missing (0) in frame 0, then
    2 + 0.05 * noise; (b) an outlier (5) in frame 0, then constant. With sums shifted by the
    first frame alone q and a*a/T cancel by a factor of about T: that kernel gave M2 off by
    1.5e-5 to 3.1e-4 of its value on these columns (1.5 to 31 times SUM). The kernel
    now sums such a column again about its mean. (c) puts the first frame where that decision
    falls (oracle/head_cases.py cond_clip): columns either side of it hold SUM too."""
    from shiftgcn import ops
    x = hc.cond_clip(clip, kind)
    dx = _dev(x)
    with _guard("head_moments"):
        part = ops.head_moments(dx)
    _check_sums(part.cpu(), hr.head_moments(x), f"head_moments column ({kind}) T{clip[2]}")
    assert torch.equal(dx.cpu(), x)


# --------------------------------------------------------------------------------------
# pooling
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.POOL_CASES, ids=_id)
def test_pool(case):
    from shiftgcn import ops
    N, M, C, P = case
    shape = (N * M, C, P, 1)
    x, dout = sc.t(shape, 21, 1.0, 0.5), sc.t((N, C), 22, 1.0, 0.25)
    d_x, d_dout = _dev(x), _dev(dout)
    with _guard("pool"):
        out = ops.pool(d_x, N, M)
    _check(out.cpu(), hr.pool(x, N, M), SUM, "pool")
    with _guard("pool_bwd"):
        dx = ops.pool_bwd(d_dout, shape, N, M)
    with _guard("pool_bwd_planes"):
        dp = ops.pool_bwd(d_dout, shape, N, M, planes=True)
    f32 = torch.from_numpy(hr.pool_bwd_planes_f32(dout, M, P))
    assert dp.shape == (N * M, C) and torch.equal(dp.cpu(), f32), "pool_bwd_planes bits"
    dxc = dx.cpu().view(N * M, C, P)
    assert torch.equal(dxc, torch.from_numpy(hr.pool_bwd_f32(dout, M, P))), "pool_bwd bits"
    assert torch.equal(dxc, dp.cpu()[:, :, None].expand(N * M, C, P))
    _check(dxc, hr.pool_bwd(dout, M, P), E6, "pool_bwd")
    _check(dp.cpu(), hr.pool_bwd_planes(dout, M, P), E6, "pool_bwd_planes")
    assert torch.equal(d_x.cpu(), x) and torch.equal(d_dout.cpu(), dout)


def test_pool_bwd_refuses_misaligned_destination():
    L, lib = _lib()
    N, M, C, P = 2, 2, 3, 7
    d_dout = _dev(sc.t((N, C), 22))
    g = _Guarded()
    dx = g.empty((N * M * C * P + 3,), device=DEV)
    assert dx.data_ptr() % 16 == 0
    for off in (4, 8, 12):
        assert lib.sgcn_pool_bwd(_p(d_dout), _p(dx, off), N, M, C, P, _stream()) == L.EINVAL
    torch.cuda.synchronize()
    g.assert_nothing_written("pool_bwd, misaligned dx")
    assert lib.sgcn_pool_bwd(_p(d_dout), _p(dx), N, M, C, P, _stream()) == 0
    g.assert_margins("pool_bwd")
    assert bool((dx[N * M * C * P:].view(torch.int32) == SENTINEL).all())


# --------------------------------------------------------------------------------------
# sgcn_bn_finalize
# --------------------------------------------------------------------------------------
def _run_finalize(part, B, F, n_part, perm_V, gamma, beta, momentum, rm0, rv0, tag):
    """One sgcn_bn_finalize launch against hr.bn_finalize; gamma / beta, rm0 / rv0 may be None."""
    L, lib = _lib()
    d_part, d_gamma, d_beta = _dev(part), _dev(gamma), _dev(beta)
    g = _Guarded()
    out = [g.empty((F,), device=DEV) for _ in range(4)]
    rm = rv = nb = None
    if rm0 is not None:
        rm, rv = g.empty((F,), device=DEV), g.empty((F,), device=DEV)
        nb = g.empty((1,), device=DEV, dtype=torch.int64)
        rm.copy_(rm0)
        rv.copy_(rv0)
        nb.fill_(41)
    rc = lib.sgcn_bn_finalize(_p(d_part), B, F, n_part, perm_V, _p(d_gamma), _p(d_beta), EPS,
                              momentum, _p(rm), _p(rv), _p(nb), *map(_p, out), _stream())
    assert rc == 0, (tag, rc)
    g.assert_margins(tag)
    ref = hr.bn_finalize(part, B, n_part, gamma, beta, EPS, _f(momentum), rm0, rv0, perm_V)
    for got, want, bar, what in zip(out, ref, (E6, E6, E6, E5),
                                    ("mean", "invstd", "scale", "shift")):
        _check(got.cpu(), want, bar, f"{tag} {what}")
    if rm0 is not None:
        _check(rm.cpu(), ref[4], E6, tag + " running_mean")
        _check(rv.cpu(), ref[5], E6, tag + " running_var")
        assert int(nb) == 42, tag + ": num_batches advances by exactly one"
    assert torch.equal(d_part.cpu(), part)
    return [o.cpu() for o in out]


def _finalize_operands(B, F, n_part=7):
    """(part, gamma, beta, running mean, running variance). Signs chosen so that no output of a
    single feature (F = 1 is its own vector) is a cancelled difference: positive means and
    running means, negative beta (shift = beta - mean*scale)."""
    part = torch.stack((sc.t((B, F), 31, 1.0, 1.5), sc.t((B, F), 32, 0.5 * n_part, n_part)), -1)
    return (part, sc.t((F,), 33, 0.4, 1.0), sc.t((F,), 34, 0.3, -0.5), sc.t((F,), 35, 0.2, 0.5),
            sc.t((F,), 36, 0.3, 1.0))


@pytest.mark.parametrize("B", hc.FIN_B)
def test_bn_finalize(B):
    n_part = 7
    for F in hc.FIN_F:
        part, gamma, beta, rm0, rv0 = _finalize_operands(B, F, n_part)
        for perm_V in hc.fin_perm_Vs(F):
            tag = f"bn_finalize B{B} F{F} V{perm_V}"
            a = _run_finalize(part, B, F, n_part, perm_V, gamma, beta, 0.1, rm0, rv0, tag)
            _run_finalize(part, B, F, n_part, perm_V, gamma, beta, 1.0, rm0, rv0, tag + " m1")
            b = _run_finalize(part, B, F, n_part, perm_V, gamma, beta, 0.1, None, None,
                              tag + " no running")
            c = _run_finalize(part, B, F, n_part, perm_V, None, None, 0.1, rm0, rv0,
                              tag + " no affine")
            # the statistics do not depend on the optional operands
            assert all(torch.equal(u, v) for u, v in zip(a, b))
            assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
            assert torch.equal(c[2], c[1]), "scale without gamma is invstd"


def test_bn_finalize_large_means():
    """Means near 1e3 with M2 near 1e-2: the merge's sum of squared means minus the squared
    sum cancels twelve digits, which only the double merge survives."""
    B, F, n_part = 9, 65, 7
    part = torch.stack((sc.t((B, F), 41, 0.01, 1000.0), sc.t((B, F), 42, 0.005, 0.01)), -1)
    _, gamma, beta, rm0, rv0 = _finalize_operands(B, F)
    _run_finalize(part, B, F, n_part, 0, gamma, beta, 0.1, rm0, rv0, "bn_finalize large means")


def test_bn_finalize_single_element():
    """B = 1, n_part = 1: no unbiased variance; the running variance takes the biased one."""
    F = 65
    part = torch.stack((sc.t((1, F), 43, 1.0, 0.5), torch.zeros(1, F)), -1)
    _, gamma, beta, rm0, rv0 = _finalize_operands(1, F)
    for perm_V in (0, 5):
        _run_finalize(part, 1, F, 1, perm_V, gamma, beta, 0.1, rm0, rv0,
                      f"bn_finalize single element V{perm_V}")


def test_moments_then_finalize():
    """End to end: sgcn_moments then sgcn_bn_finalize against the float64 statistics of x.
    The statistics pass through float32 plane sums: SUM for mean, invstd and scale, E5 for
    shift."""
    from shiftgcn import ops
    L, lib = _lib()
    B, C, T, V = 9, 5, 13, 25
    x = sc.t((B, C, T, V), 44, 2.0, 0.3)
    gamma, beta = sc.t((C,), 45, 0.4, 1.0), sc.t((C,), 46, 0.3)
    d_x, d_gamma, d_beta = _dev(x), _dev(gamma), _dev(beta)
    with _guard("moments"):
        part = ops.moments(d_x, 0)
    g = _Guarded()
    out = [g.empty((C,), device=DEV) for _ in range(4)]
    rc = lib.sgcn_bn_finalize(_p(part), B, C, T * V, 0, _p(d_gamma), _p(d_beta), EPS, 0.1, None,
                              None, None, *map(_p, out), _stream())
    assert rc == 0
    g.assert_margins("finalize")
    xd = x.double()
    mean = xd.mean((0, 2, 3))
    invstd = (xd.var((0, 2, 3), unbiased=False) + EPS).rsqrt()
    scale = gamma.double() * invstd
    for got, want, bar, what in zip(out, (mean, invstd, scale, beta.double() - mean * scale),
                                    (SUM, SUM, SUM, E5), ("mean", "invstd", "scale", "shift")):
        _check(got.cpu(), want, bar, "moments + finalize " + what)


# --------------------------------------------------------------------------------------
# sgcn_bn_bwd_finalize
# --------------------------------------------------------------------------------------
def _run_bwd_finalize(part, B, F, n_total, perm_V, mean, invstd, gamma, acc, batch_stats,
                      want_grads, tag):
    L, lib = _lib()
    d = [_dev(v) for v in (part, mean, invstd, gamma)]
    g = _Guarded()
    coef = g.empty((3, F), device=DEV)
    dg = db = None
    if want_grads:
        dg, db = g.empty((F,), device=DEV), g.empty((F,), device=DEV)
        if acc is not None:
            dg.copy_(acc[0])
            db.copy_(acc[1])
    rc = lib.sgcn_bn_bwd_finalize(_p(d[0]), B, F, n_total, perm_V, _p(d[1]), _p(d[2]), _p(d[3]),
                                  _p(dg), _p(db), int(acc is not None), int(batch_stats),
                                  _p(coef), _stream())
    assert rc == 0, (tag, rc)
    g.assert_margins(tag)
    rdg, rdb, rcoef = hr.bn_bwd_finalize(part, n_total, perm_V, mean, invstd, gamma, acc,
                                         batch_stats)
    if want_grads:
        _check(dg.cpu(), rdg, E6, tag + " dgamma")
        _check(db.cpu(), rdb, E6, tag + " dbeta")
    coef = coef.cpu()
    _check(coef[0], rcoef[0], E6, tag + " k1")
    if batch_stats:
        _check(coef[1], rcoef[1], E6, tag + " k2")
        _check(coef[2], rcoef[2], E5, tag + " k3")
    else:       # a fixed affine map: k2 = k3 = +0 exactly
        assert bool((coef[1:].view(torch.int32) == 0).all()), tag + ": k2, k3 are not +0"
    return coef


@pytest.mark.parametrize("B", hc.FIN_B)
def test_bn_bwd_finalize(B):
    n_total = B * 7
    for F in hc.FIN_F:
        part = sc.t((B, F, 2), 51, 1.0, 0.3)
        mean, invstd, gamma = sc.t((F,), 52, 0.3), sc.t((F,), 53, 0.4, 1.0), sc.t((F,), 54, 0.4, 1.0)
        acc = (sc.t((F,), 55), sc.t((F,), 56))
        for perm_V in hc.fin_perm_Vs(F):
            tag = f"bn_bwd_finalize B{B} F{F} V{perm_V}"
            run = lambda gm, ac, bs, wg, t: _run_bwd_finalize(
                part, B, F, n_total, perm_V, mean, invstd, gm, ac, bs, wg, tag + t)
            a = run(gamma, None, True, True, "")
            b = run(gamma, acc, True, True, " accumulate")
            c = run(gamma, None, True, False, " no grads")
            assert torch.equal(a, b) and torch.equal(a, c)
            run(gamma, None, False, True, " eval")
            run(None, acc, True, True, " no gamma")


# --------------------------------------------------------------------------------------
# sgcn_sgd_step with the raw table
# --------------------------------------------------------------------------------------
class _SgdArena:
    """Parameters, gradients and momentum buffers of hc.SGD_NUMEL carved from one arena each,
    at odd element offsets, the rest of every arena holding the sentinel."""

    def __init__(self, first, nan_first=True):
        self.offs, self.size = hc.sgd_layout()
        self.numels = hc.SGD_NUMEL
        self.dev = []
        self.host = []
        for j, (scale, offset) in enumerate(((1.0, 0.2), (0.5, 0.0), (0.3, 0.0))):
            a = torch.empty((self.size,), device=DEV)
            a.view(torch.int32).fill_(SENTINEL)
            vals = []
            for k, (o, n) in enumerate(zip(self.offs, self.numels)):
                v = sc.t((n,), 300 + 100 * j + k, scale, offset)
                if j == 2 and first[k] and nan_first:
                    v = torch.full((n,), float("nan"))    # a new buffer must not be read
                a[o:o + n] = v.to(DEV)
                vals.append(v)
            self.dev.append(a)
            self.host.append(vals)
        self.gap = torch.ones(self.size, dtype=torch.bool)
        for o, n in zip(self.offs, self.numels):
            self.gap[o:o + n] = False
        ch = hc.sgd_chunks()
        self.n_chunks = len(ch)
        self.chunks = torch.tensor(ch, dtype=torch.int32).reshape(-1).to(DEV)
        self.numel = torch.tensor(self.numels, dtype=torch.int32).to(DEV)

    def ptrs(self):
        return [tuple(a.data_ptr() + 4 * o for a in self.dev) for o in self.offs]

    def snapshot(self):
        """[params, grads, bufs] as lists of host tensors, after checking every gap."""
        torch.cuda.synchronize()
        out = []
        for a, name in zip(self.dev, ("param", "grad", "buf")):
            h = a.cpu()
            assert bool((h.view(torch.int32)[self.gap] == SENTINEL).all()), \
                f"sgd_step wrote beside a {name} tensor"
            out.append([h[o:o + n].clone() for o, n in zip(self.offs, self.numels)])
        return out

    def bits(self, j):
        return self.dev[j].cpu().view(torch.int32).clone()


def _sgd_reference(state, wd_lr, flags, scales, momentum, nesterov):
    """hr.sgd_step per tensor on host copies [params, grads, bufs]."""
    out = ([], [], [])
    for k, (p, g, b) in enumerate(zip(*state)):
        wd, lr = (_f(v) for v in wd_lr[k])
        r = hr.sgd_step(p, g, b, wd, lr, _f(momentum), nesterov, bool(flags[k] & 1),
                        _f(scales[k]) if flags[k] & 2 else None)
        for o, v in zip(out, r):
            o.append(v)
    return out


def _sgd_compare(got, ref, before, flags, scales, momentum, tag):
    cat = lambda vs: torch.cat([v.double() for v in vs])
    _check(cat(got[0]), cat(ref[0]), E6, tag + " param")
    _check(cat(got[1]), cat(ref[2]), E6, tag + " grad")
    for k, (g1, g0) in enumerate(zip(got[1], before[1])):
        want = g0 if not flags[k] & 2 else torch.from_numpy(g0.numpy() * np.float32(scales[k]))
        assert torch.equal(g1, want), f"{tag}: grad {k} is not g * s in float32"
    if momentum:
        _check(cat(got[2]), cat(ref[1]), E6, tag + " buf")


SGD_RUNS = [(0.9, True, False), (0.9, False, False), (0.5, True, True), (0.0, False, False),
            (0.0, False, True)]


@pytest.mark.parametrize("momentum,nesterov,wd_zero", SGD_RUNS)
def test_sgd_step_table(momentum, nesterov, wd_zero):
    L, lib = _lib()
    n = len(hc.SGD_NUMEL)
    first = [k % 2 == 1 for k in range(n)]
    flags = [int(first[k]) | (2 if k % 3 == 0 else 0) for k in range(n)]
    scales = [0.25 + 0.125 * k for k in range(n)]
    wd_lr = [(0.0 if wd_zero or k % 4 == 1 else 1e-3 * (k + 1), 0.05 + 0.01 * k)
             for k in range(n)]
    ar = _SgdArena(first)
    before = ar.snapshot()
    buf_bits = ar.bits(2)
    table = torch.from_numpy(hc.sgd_table(ar.ptrs(), wd_lr, flags, scales)).to(DEV)
    tag = f"sgd_step m{momentum} n{int(nesterov)} wd0{int(wd_zero)}"
    rc = lib.sgcn_sgd_step(_p(table), _p(ar.numel), _p(ar.chunks), ar.n_chunks, momentum,
                           int(nesterov), _stream())
    assert rc == 0, rc
    got = ar.snapshot()
    ref = _sgd_reference(before, wd_lr, flags, scales, momentum, nesterov)
    _sgd_compare(got, ref, before, flags, scales, momentum, tag)
    if momentum == 0:       # no momentum: the buffers, NaN and sentinel alike, are untouched
        assert torch.equal(ar.bits(2), buf_bits), tag + ": a buffer was written"
    else:
        assert all(torch.isfinite(b).all() for b in got[2]), tag + ": a new buffer was read"


def test_sgd_step_device_hyperparameters():
    """Flags bit 2 outside capture: {weight_decay, lr} read from a device address; the pair
    changes between two launches of an unchanged table and the second launch follows it."""
    L, lib = _lib()
    n = len(hc.SGD_NUMEL)
    first = [k == 2 for k in range(n)]
    flags = [4 | int(first[k]) | (2 if k == 4 else 0) for k in range(n)]
    scales = [0.5] * n
    ar = _SgdArena(first)
    wd_lr = [(1e-3 * (k % 3), 0.1 + 0.01 * k) for k in range(n)]
    pairs = _dev(torch.tensor(wd_lr, dtype=torch.float32))
    table = torch.from_numpy(hc.sgd_table(
        ar.ptrs(), [pairs.data_ptr() + 8 * k for k in range(n)], flags, scales)).to(DEV)
    state = ar.snapshot()
    for step, hyper in enumerate((wd_lr, [(2e-3, 0.01 + 0.002 * k) for k in range(n)])):
        pairs.copy_(torch.tensor(hyper, dtype=torch.float32))
        rc = lib.sgcn_sgd_step(_p(table), _p(ar.numel), _p(ar.chunks), ar.n_chunks, 0.9, 1,
                               _stream())
        assert rc == 0, rc
        got = ar.snapshot()
        ref = _sgd_reference(state, hyper, flags, scales, 0.9, True)
        _sgd_compare(got, ref, state, flags, scales, 0.9, f"sgd_step device pair, launch {step}")
        state = got
    assert torch.equal(pairs.cpu(), torch.tensor(hyper, dtype=torch.float32))


def test_sgd_step_refusals():
    L, lib = _lib()
    assert lib.sgcn_sgd_step(None, None, None, 0, 0.9, 1, _stream()) == 0
    n = len(hc.SGD_NUMEL)
    ar = _SgdArena([False] * n)
    bits = [ar.bits(j) for j in range(3)]
    table = torch.from_numpy(hc.sgd_table(ar.ptrs(), [(1e-3, 0.1)] * n, [0] * n, [1.0] * n)).to(DEV)
    args = (_p(table), _p(ar.numel), _p(ar.chunks))
    assert lib.sgcn_sgd_step(*args, ar.n_chunks, -0.5, 0, _stream()) == L.EINVAL
    assert lib.sgcn_sgd_step(*args, -1, 0.9, 0, _stream()) == L.EINVAL
    assert lib.sgcn_sgd_step(*args, 0, 0.9, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(ar.bits(j), bits[j]) for j in range(3)), "a refused step wrote"
    assert lib.sgcn_sgd_chunk_elems() == hc.SGD_CHUNK


# --------------------------------------------------------------------------------------
# sgcn_modalities
# --------------------------------------------------------------------------------------
SUBSETS = [(0,), (1,), (2,), (3,), (0, 1, 2, 3)]


def _run_modalities(d_joint, d_par, subset, scale, shift, planes, dims):
    L, lib = _lib()
    N, C, T, V, M = dims
    g = _Guarded()
    shape = (N * M, C, T, V) if planes else (N, C, T, V, M)
    outs = [g.empty(shape, device=DEV) if k in subset else None for k in range(4)]
    rc = lib.sgcn_modalities(_p(d_joint), _p(d_par), *map(_p, outs), _p(scale), _p(shift),
                             int(planes), N, C, T, V, M, _stream())
    return rc, outs, g


@pytest.mark.parametrize("V,M", hc.MOD_VM, ids=lambda v: str(v))
def test_modalities(V, M):
    par = hc.synthetic_parent(V)
    d_par = torch.from_numpy(par).to(DEV)
    N = hc.MOD_N
    for C in hc.MOD_C:
        for T in hc.MOD_T:
            dims = (N, C, T, V, M)
            F = M * V * C
            joint = sc.t(dims, 600 + 10 * C + T, 1.0, 0.1)
            scale, shift = sc.t((4, F), 61, 0.5, 1.0), sc.t((4, F), 62, 0.3)
            d_joint, d_scale, d_shift = _dev(joint), _dev(scale), _dev(shift)
            aff = hr.modalities(joint, par, scale, shift, planes=True)
            for planes in (False, True):
                exact = hr.modalities_f32(joint, par, planes=planes)
                f64 = hr.modalities(joint, par, planes=planes)
                for subset in SUBSETS:
                    tag = f"modalities C{C} T{T} planes{int(planes)} {subset}"
                    rc, outs, g = _run_modalities(d_joint, d_par, subset, None, None, planes, dims)
                    assert rc == 0, (tag, rc)
                    g.assert_margins(tag)
                    for k in subset:
                        assert torch.equal(outs[k].cpu(), exact[k]), f"{tag}: stream {k} bits"
                    if len(subset) == 4:
                        for k in subset:
                            _check(outs[k].cpu(), f64[k], E6, f"{tag} stream {k}")
            for subset in SUBSETS:
                tag = f"modalities C{C} T{T} data_bn {subset}"
                rc, outs, g = _run_modalities(d_joint, d_par, subset, d_scale, d_shift, True, dims)
                assert rc == 0, (tag, rc)
                g.assert_margins(tag)
                for k in subset:
                    _check(outs[k].cpu(), aff[k], E6, f"{tag} stream {k}")
            assert torch.equal(d_joint.cpu(), joint)


def test_modalities_refusals_and_empty_batch():
    L, lib = _lib()
    V, M, C, T, N = 7, 3, 3, 2, 2
    dims = (N, C, T, V, M)
    d_par = torch.from_numpy(hc.synthetic_parent(V)).to(DEV)
    d_joint = _dev(sc.t(dims, 63))
    d_scale, d_shift = _dev(sc.t((4, M * V * C), 61, 0.5, 1.0)), _dev(sc.t((4, M * V * C), 62))
    full = SUBSETS[-1]
    for what, (s, h, planes) in {"scale without shift": (d_scale, None, True),
                                 "shift without scale": (None, d_shift, True),
                                 "data_bn with planes = 0": (d_scale, d_shift, False)}.items():
        rc, outs, g = _run_modalities(d_joint, d_par, full, s, h, planes, dims)
        assert rc == L.EINVAL, (what, rc)
        torch.cuda.synchronize()
        g.assert_nothing_written(what)
    # N = 0: nothing to read or write; the pointers may be NULL
    g = _Guarded()
    outs = [g.empty((8,), device=DEV) for _ in range(4)]
    for planes in (0, 1):
        assert lib.sgcn_modalities(None, None, *map(_p, outs), None, None, planes, 0, C, T, V, M,
                                   _stream()) == 0
    torch.cuda.synchronize()
    g.assert_nothing_written("modalities N = 0")
