"""The bf16-operand forward contraction (sgcn_pw_fwd_bf16, pwconv.hip: pwg_fwd_bf16_kernel)
against the float64 restatement (oracle/pw_ref.py pw_fwd_ref) on operands THE TEST has
rounded to bf16 (weight and X, tests/bf16_cases.py round_bf16), on every tile of
kPwBf16Tiles.

Bar: |got - ref| <= 1e-5 + 1e-5 * |ref|, the fp32 kernel's bar (tests/test_gpu_pw_ref.py):
the products of two bf16 values are exact in fp32, so only the accumulation rounds, as in
the fp32 kernel. Each figure is printed before it is asserted (_check).

Operands sit in poisoned allocations like those of tests/test_gpu_pw_ref.py: inputs in NaN,
outputs in a sentinel bit pattern; a result must equal the reference wherever the header's
addressing formula writes and keep the sentinel, bit for bit, everywhere else.

Not pinned: subnormal, infinite and NaN operands.

Rounding-mode test, -0.0: the contraction's sum starts from +0.0, and (+0.0) + (-0.0) is
+0.0 under round to nearest, so the expected output for x = -0.0 is +0.0 (the fp32 kernel's
signed-zero test pins the same rule); every other element must be round_bf16(x) bit for bit.
"""
import pytest
import torch

import bf16_cases as bc
from bf16_cases import pc, pr, round_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda"
E5 = 1e-5
SENTINEL = 0x7FC12345      # a quiet NaN with a payload: any rewrite of it shows in the bits


def _id(s):
    return "x".join(map(str, s))


def _check(got, ref, rtol, atol, what):
    """|got - ref| <= atol + rtol*|ref| everywhere; the figures are printed first."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(ref).all(), what
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    used = float((err / (atol + rtol * ref.abs())).max())
    print(f"{what}: max err {float(err.max()):.3e} max|ref| {float(ref.abs().max()):.3e} "
          f"bar use {used:.3f} (rtol {rtol:.0e} atol {atol:.1e})")
    assert used <= 1.0, (what, float(err.max()), used)


class _Op:
    """One plane operand inside a poisoned allocation (NaN around inputs, the sentinel
    around and under outputs); ``view``: a batch / channel / row slice of a larger tensor."""

    def __init__(self, B, C, T, V, tstride, rsign, view, data=None, out=False):
        rows = (T - 1) * tstride + 1
        shape = (B + 2, C + 3, rows + 2, V) if view else (B, C, rows, V)
        self.big = torch.empty(shape, device=DEV)
        if out:
            self.big.view(torch.int32).fill_(SENTINEL)
        else:
            self.big.fill_(float("nan"))
        self.t = self.big[1:1 + B, 2:2 + C, 1:1 + rows] if view else self.big
        self.ref = pr.Plane(self.t, tstride, rsign)
        self.idx = self.ref.index(B, C, T, V)
        if data is not None:
            self.ref.flat()[self.idx] = data.to(DEV)
        self.before = self.ref.flat().clone()

    def view(self):
        from shiftgcn import ops
        return ops.PlaneView(self.t, self.ref.tstride, self.ref.rsign)

    def assert_surroundings_untouched(self, what):
        flat = self.ref.flat()
        keep = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
        keep[self.idx.reshape(-1)] = False
        assert torch.equal(flat.view(torch.int32)[keep], self.before.view(torch.int32)[keep]), \
            f"{what}: an element outside the logical plane was written"


def _run(M, K, plane, w_mcontig=False, relu=True, bias=True, y_rsign=0, view=False, x_tstride=1,
         y_tstride=1, xdata=None, wdata=None, bdata=None, exact=False, seed=0):
    """One launch against the float64 reference on rounded operands; returns the logical
    output (B, M, T, V)."""
    from shiftgcn import ops
    B, T, V = plane
    sd = 1000 * M + 10 * K + V + seed
    xd = pc.rnd((B, K, T, V), sd) if xdata is None else xdata
    w = (pc.rnd((K, M) if w_mcontig else (M, K), sd + 2, K ** -0.5) if wdata is None
         else wdata).to(DEV)
    b = None
    if bias:
        b = (pc.rnd((M,), sd + 3) if bdata is None else bdata).to(DEV)
    x = _Op(B, K, T, V, x_tstride, 0, view, data=xd)
    y = _Op(B, M, T, V, y_tstride, y_rsign, view, out=True)
    xr = pr.Plane(round_bf16(xd).to(DEV))                  # the rounded logical operand
    flat, idx = pr.pw_fwd_ref(round_bf16(w), w_mcontig, b, xr, y.ref, M, K, T, V, relu=relu)
    ops.pw_fwd_bf16(w, w_mcontig, b, x.view(), y.view(), M, K, T, V, relu=relu)
    what = (f"pw_fwd_bf16 {bc.bf16_form(M, K)[:2]} M{M}K{K}p{_id(plane)} a{int(w_mcontig)}"
            f"r{int(relu)}b{int(bias)}y{y_rsign} ts{x_tstride}{y_tstride} v{int(view)}")
    got = y.ref.flat()[idx]
    if exact:
        assert torch.equal(got.view(torch.int32), flat[idx].float().view(torch.int32)), what
    else:
        _check(got, flat[idx], E5, E5, what)
    y.assert_surroundings_untouched(what)
    assert torch.equal(x.ref.flat().view(torch.int32), x.before.view(torch.int32))
    return got


@pytest.mark.parametrize("plane", bc.FWD_PLANES, ids=_id)
@pytest.mark.parametrize("M", bc.BF16_MS)
def test_sizes(M, plane):
    """Every M (exact and ragged at each tile edge, two row blocks at 300) x every K (around
    the MFMA k-step, the stage and the limit) x every plane; k- and m-contiguous weights."""
    for i, K in enumerate(bc.BF16_KS):
        _run(M, K, plane, w_mcontig=bool(i & 1), relu=bool(i & 2))
        _run(M, K, plane, w_mcontig=not (i & 1), relu=False, bias=False)


@pytest.mark.parametrize("c", bc.flag_cases(),
                         ids=lambda c: f"M{c['M']}K{c['K']}a{int(c['w_mcontig'])}r{int(c['relu'])}"
                                       f"b{int(c['bias'])}y{c['y_rsign']}")
def test_flags(c):
    """w_mcontig x relu x bias / None x y_rsign in {-1, 0, +1} on one ragged (M, K) per tile."""
    _run(**c)


@pytest.mark.parametrize("tile", list(bc.BF16_FLAG_PAIRS), ids=_id)
@pytest.mark.parametrize("xt,yt", [(2, 1), (1, 2), (2, 2)])
def test_time_strides(tile, xt, yt):
    """x_tstride = 2 (the strided residual conv) and y_tstride = 2, on allocations that end
    with the last logical row and as slices of larger poisoned tensors."""
    M, K = bc.BF16_FLAG_PAIRS[tile]
    for view in (False, True):
        _run(M, K, (3, 13, 25), view=view, x_tstride=xt, y_tstride=yt)
        _run(M, K, (2, 9, 33), w_mcontig=True, y_rsign=1, view=view, x_tstride=xt, y_tstride=yt)


@pytest.mark.parametrize("tile", list(bc.BF16_FLAG_PAIRS), ids=_id)
def test_views_with_poisoned_surroundings(tile):
    """Non-contiguous batch / channel strides with storage offsets: every operand a slice of
    a larger tensor, NaN around the input, the sentinel around the output."""
    M, K = bc.BF16_FLAG_PAIRS[tile]
    for plane in ((3, 13, 25), (1, 2, 25)):
        _run(M, K, plane, view=True)
        _run(M, K, plane, w_mcontig=True, y_rsign=-1, relu=False, bias=False, view=True)


@pytest.mark.parametrize("tile", list(bc.BF16_EXACT), ids=_id)
def test_exact_integers(tile):
    """Integer operands in [-4, 4] and an integer bias: every partial sum is below 2^24, so
    the result equals the integer contraction bit for bit whatever the summation order."""
    M, K = bc.BF16_EXACT[tile]
    B, T, V = 2, 7, 25
    g = torch.Generator().manual_seed(M + K)
    xi = torch.randint(-4, 5, (B, K, T, V), generator=g).float()
    bi = torch.randint(-9, 10, (M,), generator=g).float()
    for amc in (False, True):
        wi = torch.randint(-4, 5, (K, M) if amc else (M, K), generator=g).float()
        got = _run(M, K, (B, T, V), w_mcontig=amc, relu=False, xdata=xi, wdata=wi, bdata=bi,
                   exact=True)
        assert float(got.abs().max()) > 16 and float(got.abs().max()) < 2 ** 24


def test_rounding_mode_is_nearest_even():
    """M = 5, K = 1, A = 1, no bias: the output is the kernel's rounding of X itself. bf16
    ties and near-ties of both signs (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6, and their
    neighbours one fp32 ulp either side), -0.0 (see the header), large and small normals."""
    from shiftgcn import ops
    u = 2.0 ** -23
    vals = []
    for base in (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8):
        vals += [base, base - u, base + u]
    vals += [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -7 - u, 3.0e38, 1.0e38 * (1 + 2.0 ** -8), 1.5e-38,
             2.0 ** -120 * (1 + 3 * 2.0 ** -8), 255.5, 0.1, 1.0 / 3.0, 65504.0, 0.0]
    vals = vals + [-v for v in vals]                       # both signs; -0.0 among them
    x32 = torch.tensor(vals, dtype=torch.float64).float()
    assert torch.signbit(x32[-1]) and float(x32[-1]) == 0.0
    T, V = -(-len(vals) // 25), 25
    xd = torch.ones(T * V)
    xd[:len(vals)] = x32
    xd = xd.view(1, 1, T, V)
    want = round_bf16(xd)
    # the ties really are ties, and they go to even
    assert float(want[0, 0, 0, 0]) == 1.0 and float(want[0, 0, 0, 3]) == 1 + 2.0 ** -6
    x = _Op(1, 1, T, V, 1, 0, False, data=xd)
    y = _Op(1, 5, T, V, 1, 0, False, out=True)
    w = torch.ones(5, 1, device=DEV)
    ops.pw_fwd_bf16(w, False, None, x.view(), y.view(), 5, 1, T, V, relu=False)
    got = y.ref.flat()[y.idx].cpu()
    expect = (want + 0.0).expand(1, 5, T, V)               # the sum starts from +0.0
    for i in range(len(vals)):
        print(f"x {float(xd.view(-1)[i])!r:>24} -> {float(got[0, 0].view(-1)[i])!r:>24} "
              f"(round_bf16 {float(want.view(-1)[i])!r})")
    assert torch.equal(got.view(torch.int32), expect.contiguous().view(torch.int32))
    nz = xd.expand(1, 5, T, V) != 0
    assert torch.equal(got[nz].view(torch.int32),
                       want.expand(1, 5, T, V)[nz].contiguous().view(torch.int32))


@pytest.mark.parametrize("tile", list(bc.BF16_FLAG_PAIRS), ids=_id)
def test_operands_already_in_bf16_are_not_changed_again(tile):
    """The launch on (w, x) and the launch on the test's own round_bf16(w), round_bf16(x)
    give the same bits: a missing conversion (or one that is not round to nearest even)
    changes the first, a double or lossy one the second."""
    from shiftgcn import ops
    from shiftgcn.ops import PlaneView as PV
    M, K = bc.BF16_FLAG_PAIRS[tile]
    B, T, V = 3, 13, 25
    x = pc.rnd((B, K, T, V), 5).to(DEV)
    bias = pc.rnd((M,), 7).to(DEV)
    for amc in (False, True):
        w = pc.rnd((K, M) if amc else (M, K), 6, K ** -0.5).to(DEV)
        y0 = torch.empty(B, M, T, V, device=DEV)
        y1 = torch.empty_like(y0)
        ops.pw_fwd_bf16(w, amc, bias, PV(x), PV(y0), M, K, T, V)
        ops.pw_fwd_bf16(round_bf16(w), amc, bias, PV(round_bf16(x)), PV(y1), M, K, T, V)
        assert torch.equal(y0, y1)
        assert not torch.equal(round_bf16(x), x)
        # and it is not the fp32 contraction of the unrounded operands
        y2 = torch.empty_like(y0)
        ops.pw_fwd(w, amc, bias, PV(x), PV(y2), M, K, T, V)
        assert not torch.equal(y0, y2)


def test_batch_chunking_is_bit_identical(monkeypatch):
    from shiftgcn import ops
    from shiftgcn.ops import PlaneView as PV
    M, K, B, T, V = 130, 37, 5, 7, 25
    x = pc.rnd((B, K, T, V), 1).to(DEV)
    w = pc.rnd((M, K), 2, K ** -0.5).to(DEV)
    bias = pc.rnd((M,), 3).to(DEV)
    whole = torch.empty(B, M, T, V, device=DEV)
    parts = torch.empty_like(whole)
    ops.pw_fwd_bf16(w, False, bias, PV(x), PV(whole, 1, 1), M, K, T, V, relu=True)
    views = [(PV(x), K), (PV(parts), M)]
    lim = max(C * v.cstride + T * v.tstride * V + v.bstride for v, C in views) + 1
    monkeypatch.setattr(ops, "PW_MAX_ELEMS", lim)
    assert ops._batch_chunk(views, B, T, V) == 2
    ops.pw_fwd_bf16(w, False, bias, PV(x), PV(parts, 1, 1), M, K, T, V, relu=True)
    assert torch.equal(whole, parts)
