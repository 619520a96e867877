"""The contraction kernels (pwconv.hip: pwg_fwd_kernel, pw_fwd_smallm_kernel, pw_dw_kernel,
pw_dw3_kernel, pw_dw_smallc_kernel, the slab reduce and the fused temporal-shift operand)
against their float64 restatement (oracle/pw_ref.py) at every launch form.

The shapes and flag crosses (oracle/pw_cases.py) are the smallest that reach each kernel
family, tile and template instance, a split of more than one chunk, an empty trailing split,
a split that starts inside a sample and one that runs over a sample end;
tests/test_oracle_pw.py checks that coverage, and pins the restatement, without a GPU.

Every operand is laid into a poisoned allocation: inputs sit in NaN, outputs in a sentinel
bit pattern, and only the elements the header's addressing formula names hold data. In the
table tests the allocation is the operand's exact extent; the ``view`` tests make every
operand a batch / channel slice (and, under tstride = 2, the odd rows) of a larger tensor.
A result must equal the reference wherever the formula writes and keep the sentinel, bit for
bit, everywhere else: what checks the descriptor ranges and clamped rows the kernels use in
place of predicates.

Bars (|got - ref| <= atol + rtol * |ref| per element, DESIGN.md "Parity bars"):
  forward / dX            rtol 1e-5, atol 1e-5 (unit-variance inputs, weights randn / sqrt K);
  dW / dbias, P <= 1,700  rtol 1e-5, atol 1e-4 (P = B*T*V, tests/test_gpu_kernels.py's size);
  dW / dbias, P >  1,700  atol = max(1e-4, 2 x the deviation of torch's own fp32 einsum / sum
                          on the same operands from the float64 reference), never above 2e-3.
Each figure is printed before it is asserted.

Measured on an MI355X (worst case per family, error and its share of the bar): forward
3.8e-6 / 0.20 (256 x 128 and 128 x 128 at K = 256), small-M 1.8e-6 / 0.12, fused temporal
shift 3.4e-6 / 0.17; dW pw_dw_kernel 1.8e-4 / 0.15, pw_dw3_kernel 1.7e-4 / 0.08, Nc <= 4
kernel 1.9e-4 / 0.07; dbias 1.2e-4 / 0.39. torch's fp32 einsum on the same operands is
6.1e-4 .. 4.0e-3 from float64 at the cases above 1,700 positions (its sum 3.1e-5 .. 1.8e-4),
so their dW bars are 1.2e-3 .. 2e-3 (capped) and their dbias bars 1.0e-4 .. 3.6e-4.
"""
import pytest
import torch

from oracle import pw_cases as pc
from oracle import pw_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
E5 = 1e-5
DW_ATOL, DW_ATOL_MAX = 1e-4, 2e-3
SENTINEL = 0x7FC12345      # a quiet NaN with a payload: any rewrite of it shows in the bits


def _id(s):
    return "x".join(map(str, s))


def _cid(c):
    return (f"M{c['M']}K{c['K']}p{_id(c['plane'])}m{int(c['mask'])}x{c['x_rsign']}y{c['y_rsign']}"
            f"a{int(c['w_mcontig'])}c{int(c['accumulate'])}r{int(c['relu'])}b{int(c['bias'])}")


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
    """One plane operand inside a poisoned allocation. ``data`` None: an output that starts
    as the sentinel everywhere."""

    def __init__(self, B, C, T, V, tstride, rsign, view, data=None, out=False):
        rows = (T - 1) * tstride + 1
        shape = (B + 2, C + 3, rows + 2, V) if view else (B, C, rows, V)
        self.big = torch.empty(shape, device=DEV)
        if out:
            self.big.view(torch.int32).fill_(SENTINEL)
        else:
            self.big.fill_(float("nan"))
        self.t = self.big[1:1 + B, 2:2 + C, 1:1 + rows] if view else self.big
        self.dims = (B, C, T, V)
        self.ref = pr.Plane(self.t, tstride, rsign)
        self.idx = self.ref.index(B, C, T, V)
        assert self.idx.unique().numel() == self.idx.numel()
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


def _padded(n, data=None):
    """A contiguous n-element tensor between two 32-element sentinel margins."""
    buf = torch.empty(n + 64, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    if data is not None:
        buf[32:32 + n] = data.to(DEV).reshape(-1)
    return buf, buf[32:32 + n]


def _margins_intact(buf, n):
    m = buf.view(torch.int32)
    return bool((m[:32] == SENTINEL).all() and (m[32 + n:] == SENTINEL).all())


# --------------------------------------------------------------------------------------
# forward / dX
# --------------------------------------------------------------------------------------
def _run_fwd(c, view=False, x_tstride=1, y_tstride=1, seed=0):
    from shiftgcn import ops
    M, K = c["M"], c["K"]
    B, T, V = c["plane"]
    sd = 1000 * M + 10 * K + V + seed
    x = _Op(B, K, T, V, x_tstride, c["x_rsign"], view, data=pc.rnd((B, K, T, V), sd))
    y = _Op(B, M, T, V, y_tstride, c["y_rsign"], view, out=True,
            data=pc.rnd((B, M, T, V), sd + 1) if c["accumulate"] else None)
    w = pc.rnd((K, M) if c["w_mcontig"] else (M, K), sd + 2, K ** -0.5).to(DEV)
    bias = pc.rnd((M,), sd + 3).to(DEV) if c["bias"] else None
    mask = pc.mask_values(V, K, sd + 4).to(DEV) if c["mask"] else None
    flat, idx = pr.pw_fwd_ref(w, c["w_mcontig"], bias, x.ref, y.ref, M, K, T, V, mask=mask,
                              relu=c["relu"], accumulate=c["accumulate"])
    ops.pw_fwd(w, c["w_mcontig"], bias, x.view(), y.view(), M, K, T, V, mask=mask,
               relu=c["relu"], accumulate=c["accumulate"])
    what = f"pw_fwd {pc.fwd_case_form(c)[:3]} {_cid(c)}"
    _check(y.ref.flat()[idx], flat[idx], E5, E5, what)
    y.assert_surroundings_untouched(what)
    assert torch.equal(x.ref.flat().view(torch.int32), x.before.view(torch.int32))


def _fwd_case(M, K, plane, **kw):
    c = dict(M=M, K=K, plane=plane, mask=False, x_rsign=0, y_rsign=0, w_mcontig=False,
             accumulate=False, relu=True, bias=True)
    c.update(kw)
    return c


@pytest.mark.parametrize("plane", pc.FWD_PLANES, ids=_id)
@pytest.mark.parametrize("MK", pc.FWD_PAIRS, ids=_id)
def test_pw_fwd_table(MK, plane):
    """Every (M, K) pair on every plane: plain, and Shift_gcn's form (shift_in gather, mask
    where V allows one, m-contiguous weights, shift_out placement)."""
    M, K = MK
    _run_fwd(_fwd_case(M, K, plane))
    _run_fwd(_fwd_case(M, K, plane, mask=plane[2] <= pc.K_MASK_MAX_V, x_rsign=1, y_rsign=1,
                       w_mcontig=True, relu=False))


@pytest.mark.parametrize("c", pc.fwd_flag_cases(), ids=_cid)
def test_pw_fwd_every_template_instance(c):
    """All 16 (MASK, XROT, AMC, ACCUM) instances of each (tile, staging), the four of the
    small-M kernel; relu on and off, bias = None among them; accumulating launches start
    from unit-variance contents and keep the same bar."""
    _run_fwd(c)


@pytest.mark.parametrize("c", pc.fwd_rsign_cases(), ids=_cid)
def test_pw_fwd_rotation_signs(c):
    _run_fwd(c)


@pytest.mark.parametrize("key", list(pc.FWD_FLAG_PAIRS) + ["smallm"], ids=str)
@pytest.mark.parametrize("xt,yt", [(1, 1), (2, 1), (1, 2)])
def test_pw_fwd_views_with_poisoned_surroundings(key, xt, yt):
    """Every operand a batch / channel slice of a larger tensor (under tstride = 2 its odd
    rows), NaN around the inputs, the sentinel around the output (rows at or past M, the even
    rows, the other batch and channel slices): one case per kernel family and tile, plain
    and rotated + masked + accumulating."""
    M, K = pc.SMALLM_PAIRS[0] if key == "smallm" else pc.FWD_FLAG_PAIRS[key]
    for plane in ((3, 13, 25), (1, 2, 25)):
        _run_fwd(_fwd_case(M, K, plane), view=True, x_tstride=xt, y_tstride=yt)
        if key == "smallm":
            _run_fwd(_fwd_case(M, K, plane, w_mcontig=True, accumulate=True, bias=False),
                     view=True, x_tstride=xt, y_tstride=yt)
        else:
            _run_fwd(_fwd_case(M, K, plane, mask=True, x_rsign=1, y_rsign=-1, w_mcontig=True,
                               accumulate=True), view=True, x_tstride=xt, y_tstride=yt)


@pytest.mark.parametrize("key", list(pc.FWD_FLAG_PAIRS) + ["smallm"], ids=str)
def test_pw_fwd_time_strides_exact_extent(key):
    """x_tstride = 2 and y_tstride = 2 on allocations that end with the last logical row."""
    M, K = pc.SMALLM_PAIRS[0] if key == "smallm" else pc.FWD_FLAG_PAIRS[key]
    for xt, yt in ((2, 1), (1, 2), (2, 2)):
        _run_fwd(_fwd_case(M, K, (2, 9, 33), bias=False, relu=False), x_tstride=xt, y_tstride=yt)
        _run_fwd(_fwd_case(M, K, (3, 13, 25), w_mcontig=True, accumulate=True), x_tstride=xt,
                 y_tstride=yt)


@pytest.mark.parametrize("MK", [(37, 51), (37, 100), (100, 37), (130, 37), (3, 64)], ids=_id)
def test_pw_fwd_signed_zeros_and_relu_bits(MK):
    """Small-integer operands: every sum is exact in fp32, so the output equals the float64
    formula BIT FOR BIT, signed zeros included. Rows of zero weights times negative inputs
    give -0.0 products, cancelling rows give exact zero sums, bias holds -0.0 and +0.0, and
    the accumulated-into contents hold -0.0, +0.0 and negative values: ReLU must store +0.0
    for every pre-activation <= 0 (never -0.0, never the negative), and -0.0 + (+0.0) under
    accumulate is +0.0."""
    from shiftgcn import ops
    M, K = MK
    B, T, V = 2, 7, 25
    g = torch.Generator().manual_seed(M + K)
    xi = torch.randint(-3, 4, (B, K, T, V), generator=g).float()
    wi = torch.randint(-2, 3, (M, K), generator=g).float()
    wi[0::4] = 0.0                                   # zero rows: products +-0.0
    wi[1::4, 1::2] = -wi[1::4, 0:2 * (K // 2):2]     # pairs of opposite weights ...
    xi[:, 1::2] = xi[:, 0:2 * (K // 2):2]            # ... on equal inputs: exact cancellation
    if K % 2:
        wi[1::4, K - 1] = 0.0
    bias = torch.tensor([-0.0, 0.0, 1.0, -1.0]).repeat(M)[:M].contiguous()
    old = torch.tensor([-0.0, 0.0, -2.0, 3.0, -0.0]).repeat(B * M * T * V)[:B * M * T * V]
    old = old.view(B, M, T, V)
    for relu in (True, False):
        for acc in (False, True):
            x = _Op(B, K, T, V, 1, 0, False, data=xi)
            y = _Op(B, M, T, V, 1, 0, False, out=True, data=old if acc else None)
            w, bs = wi.to(DEV), bias.to(DEV)
            flat, idx = pr.pw_fwd_ref(w, False, bs, x.ref, y.ref, M, K, T, V, relu=relu,
                                      accumulate=acc)
            ops.pw_fwd(w, False, bs, x.view(), y.view(), M, K, T, V, relu=relu, accumulate=acc)
            want = flat[idx].float()
            got = y.ref.flat()[idx]
            assert (want == 0).any() and (want > 0).any()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (relu, acc)
            if relu and not acc:
                assert not torch.signbit(got).any()


# --------------------------------------------------------------------------------------
# weight gradient
# --------------------------------------------------------------------------------------
_REF = {}


def _dw_operands(shape, g_rsign, x_rsign, mask, view=False, g_tstride=1, x_tstride=1):
    B, M, Nc, T, V = shape
    sd = 7 * M + 3 * Nc + T + V
    g = _Op(B, M, T, V, g_tstride, g_rsign, view, data=pc.rnd((B, M, T, V), sd))
    x = _Op(B, Nc, T, V, x_tstride, x_rsign, view, data=pc.rnd((B, Nc, T, V), sd + 1))
    mk = pc.mask_values(V, Nc, sd + 2).to(DEV) if mask else None
    return g, x, mk


def _dw_reference(shape, g, x, mk):
    """(dw, dbias, atol_dw, atol_db) of the logical operands: shared by every case whose
    logical G, X' are the same (the placement flags do not change them)."""
    B, M, Nc, T, V = shape
    key = (shape, mk is not None)
    if key not in _REF:
        dw, db = pr.pw_dw_ref(pr.Plane(g.ref.read(B, M, T, V)), pr.Plane(x.ref.read(B, Nc, T, V)),
                              M, Nc, T, V, mask=mk)
        a_dw = a_db = DW_ATOL
        if B * T * V > pc.DW_FIXED_BAR_POSITIONS:
            G32 = g.ref.read(B, M, T, V).float()
            X32 = pr._masked(x.ref.read(B, Nc, T, V), mk, Nc, V).float()
            d_dw = float((torch.einsum("bmtv,bctv->mc", G32, X32).double() - dw).abs().max())
            d_db = float((G32.sum((0, 2, 3)).double() - db).abs().max())
            a_dw = min(max(DW_ATOL, 2 * d_dw), DW_ATOL_MAX)
            a_db = min(max(DW_ATOL, 2 * d_db), DW_ATOL_MAX)
            print(f"fp32 torch deviation at {shape} mask{int(mk is not None)}: "
                  f"dW {d_dw:.3e} dbias {d_db:.3e} -> atol {a_dw:.2e} / {a_db:.2e}")
        _REF[key] = (dw, db, a_dw, a_db)
    return _REF[key]


def _run_dw(shape, g_rsign=0, x_rsign=0, mask=False, dbias=True, transpose=False,
            accumulate=False, dbias_accumulate=False, view=False, g_tstride=1, x_tstride=1,
            twice=False):
    from shiftgcn import ops
    B, M, Nc, T, V = shape
    g, x, mk = _dw_operands(shape, g_rsign, x_rsign, mask, view, g_tstride, x_tstride)
    dw_ref, db_ref, a_dw, a_db = _dw_reference(shape, g, x, mk)
    old_w = pc.rnd((Nc, M) if transpose else (M, Nc), 5, 3.0) if accumulate else None
    old_b = pc.rnd((M,), 6, 3.0) if dbias_accumulate else None
    wbuf, dw = _padded(M * Nc, old_w)
    dw = dw.view((Nc, M) if transpose else (M, Nc))
    bbuf, db = _padded(M, old_b) if dbias else (None, None)
    want_w = dw_ref.t() if transpose else dw_ref
    if accumulate:
        want_w = want_w + old_w.to(DEV).double()
    want_b = db_ref + old_b.to(DEV).double() if dbias_accumulate else db_ref
    f = pc.dw_form(B, M, Nc, T, V, mask, g_rsign, x_rsign, dbias)
    what = (f"pw_dw {f['family']} {f['tile']} {f['flags']} fast{int(f['fast'])} S{f['S']} "
            f"per{f['per']} empty{f['empty']} {_id(shape)} g{g_rsign}x{x_rsign}")

    def call():
        ops.pw_dw(g.view(), x.view(), dw, M, Nc, T, V, mask=mk, transpose=transpose,
                  accumulate=accumulate, dbias=db, dbias_accumulate=dbias_accumulate)

    call()
    _check(dw, want_w, E5, a_dw, what + " dW")
    if dbias:
        _check(db, want_b, E5, a_db, what + " dbias")
        assert _margins_intact(bbuf, M), what
    assert _margins_intact(wbuf, M * Nc), what
    for op in (g, x):
        assert torch.equal(op.ref.flat().view(torch.int32), op.before.view(torch.int32))
    if twice:
        assert not accumulate and not dbias_accumulate and f["S"] > 1
        first_w, first_b = dw.clone(), db.clone()
        dw.fill_(0), db.fill_(0)
        call()
        assert torch.equal(dw, first_w) and torch.equal(db, first_b), what


@pytest.mark.parametrize("operands", pc.DW_OPERANDS, ids=["plain", "general", "mask"])
@pytest.mark.parametrize("shape", pc.DW_TABLE, ids=_id)
def test_pw_dw_table(shape, operands):
    gr, xr, mk = operands
    _run_dw(shape, gr, xr, mk and shape[4] <= pc.K_MASK_MAX_V)


def _dw3_flag_cases():
    return [(c, mk, gr, xr, db) for key, shapes in pc.DW_FLAG_SHAPES.items() if key[0] == "dw3"
            for c in shapes for mk in (False, True) for gr in pc.RSIGNS for xr in pc.RSIGNS
            for db in (False, True)]


@pytest.mark.parametrize("shape,mask,gr,xr,dbias", _dw3_flag_cases(),
                         ids=lambda v: _id(v) if isinstance(v, tuple) else str(int(v)))
def test_pw_dw3_every_template_instance(shape, mask, gr, xr, dbias):
    """(mask, g_rsign, x_rsign in {0, +1, -1}, dbias or not): the 16 (MASK, GROT, XROT,
    BIAS) instances of each reachable pw_dw3 tile, both rotation signs on both operands."""
    _run_dw(shape, gr, xr, mask, dbias=dbias)


def _dw_sign_cases():
    return [(c, gr, xr, mk) for key, shapes in pc.DW_FLAG_SHAPES.items() if key[0] != "dw3"
            for c in shapes for gr in pc.RSIGNS for xr in pc.RSIGNS for mk in (False, True)]


@pytest.mark.parametrize("shape,gr,xr,mask", _dw_sign_cases(),
                         ids=lambda v: _id(v) if isinstance(v, tuple) else str(int(v)))
def test_pw_dw_rotation_signs(shape, gr, xr, mask):
    """pw_dw_kernel (every tile) and the Nc <= 4 kernel: both rotation signs, masked or not."""
    _run_dw(shape, gr, xr, mask)


_PLACEMENT = [dict(transpose=True), dict(accumulate=True), dict(dbias_accumulate=True),
              dict(transpose=True, accumulate=True, dbias_accumulate=True),
              dict(g_tstride=2), dict(x_tstride=2), dict(g_tstride=2, x_tstride=2, transpose=True)]


@pytest.mark.parametrize("kw", _PLACEMENT, ids=lambda k: "+".join(sorted(k)))
@pytest.mark.parametrize("key", list(pc.DW_FLAG_SHAPES), ids=str)
def test_pw_dw_placement_flags(key, kw):
    """transpose, accumulate and dbias_accumulate (from non-zero contents), g_tstride = 2
    and x_tstride = 2, on the plain and the rotated + masked operand of every tile."""
    for shape in pc.DW_FLAG_SHAPES[key]:
        _run_dw(shape, **kw)
        _run_dw(shape, 1, -1, True, **kw)


@pytest.mark.parametrize("key", list(pc.DW_FLAG_SHAPES), ids=str)
@pytest.mark.parametrize("gt,xt", [(1, 1), (2, 1), (1, 2)])
def test_pw_dw_views_with_poisoned_surroundings(key, gt, xt):
    """Both operands batch / channel slices of NaN-filled tensors (odd rows under tstride =
    2), dW and dbias between sentinel margins: the result is the reference's, so finite."""
    for shape in pc.DW_FLAG_SHAPES[key]:
        _run_dw(shape, view=True, g_tstride=gt, x_tstride=xt)
        _run_dw(shape, -1, 1, True, view=True, g_tstride=gt, x_tstride=xt, transpose=True)


_MULTI = [(8, 64, 64, 192, 25), (3, 129, 128, 171, 33), (3, 128, 128, 320, 25),
          (8, 100, 3, 656, 25)]


@pytest.mark.parametrize("shape", _MULTI, ids=_id)
def test_pw_dw_views_multi_chunk_splits(shape):
    """The view form where a split holds several chunks and trailing splits are empty."""
    _run_dw(shape, view=True)
    _run_dw(shape, 1, 1, True, view=True, x_tstride=2)


@pytest.mark.parametrize("shape", _MULTI + [(6, 100, 64, 150, 33), (2, 64, 256, 321, 25)],
                         ids=_id)
def test_pw_dw_is_deterministic(shape):
    """The same call twice (S > 1, the output cleared in between) is bit-identical."""
    _run_dw(shape, twice=True)
    _run_dw(shape, 1, -1, shape[4] <= pc.K_MASK_MAX_V, twice=True)


# --------------------------------------------------------------------------------------
# fused temporal shift
# --------------------------------------------------------------------------------------
class _St:
    def __init__(self, scale, shift):
        self.scale, self.shift = scale, shift


def _tshift_inputs(B, K, M, T, V, seed):
    """tests/test_gpu_tshift_fused.py's inputs: tiny x positions, a whole-joint x shift, a
    fractional one, |ypos| up to 3 and one channel shifted out of the plane."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, K, T, V, generator=g)
    w = (torch.randn(M, K, generator=g) / K ** 0.5).to(DEV)
    bias = torch.randn(M, generator=g).to(DEV)
    xpos = (torch.rand(K, generator=g) - 0.5) * 2e-8
    ypos = (torch.rand(K, generator=g) - 0.5) * 6
    xpos[0], ypos[0] = 1.0, 0.0
    xpos[1] = -1.5
    ypos[2] = float(T + 1)
    xpos[K - 1], ypos[K - 1] = -1.0, -2.5        # the last row: what a clamped row re-reads
    scale = (torch.rand(K, generator=g) + 0.5).to(DEV)
    shift = torch.randn(K, generator=g).to(DEV)
    return h, w, bias, xpos.to(DEV), ypos.to(DEV), scale, shift


@pytest.mark.parametrize("view", [False, True], ids=["exact", "view"])
@pytest.mark.parametrize("case", pc.TSHIFT_CASES, ids=_id)
def test_pw_fwd_tshift(case, view):
    """Against the float64 shift-then-contract reference, bit-identical to the two-launch
    form (sgcn_tshift_fwd + sgcn_pw_fwd), with and without the side output; the side output
    equals sgcn_tshift_fwd's in every element, at ragged K (rows clamped to K - 1) and at
    M > 256 (two M-blocks store it), and nothing outside the planes is written."""
    from shiftgcn import ops
    from shiftgcn.ops import PlaneView as PV
    B, K, M, T, V = case
    h, w, bias, xpos, ypos, scale, shift = _tshift_inputs(*case, seed=sum(case))
    x = _Op(B, K, T, V, 1, 0, view, data=h)
    two = ops.tshift_fwd(x.ref.read(B, K, T, V).float().contiguous(), xpos, ypos, 1, scale=scale,
                         shift=shift)
    r1 = torch.empty(B, M, T, V, device=DEV)
    ops.pw_fwd(w, False, bias, PV(two), PV(r1), M, K, T, V, relu=True)
    for side in (False, True):
        y = _Op(B, M, T, V, 1, 0, view, out=True)
        xs = _Op(B, K, T, V, 1, 0, view, out=True)
        flat, idx, S = pr.pw_fwd_tshift_ref(w, bias, x.ref, xpos, ypos, scale, shift, y.ref, M,
                                            K, T, V, relu=True)
        ops.pw_fwd_tshift(w, bias, x.view(), xpos, ypos, _St(scale, shift), y.view(), M, K, T, V,
                          relu=True, x_shifted=xs.t if side else None)
        what = f"pw_fwd_tshift {pc.tshift_form(M)} {_id(case)} side{int(side)}"
        got = y.ref.flat()[idx]
        _check(got, flat[idx], E5, E5, what)
        assert torch.equal(got, r1), what + ": not the two-launch result"
        y.assert_surroundings_untouched(what)
        xs.assert_surroundings_untouched(what + " side")
        if side:
            gs = xs.ref.flat()[xs.idx]
            assert torch.equal(gs, two), what + ": side output is not tshift_fwd's"
            _check(gs, S, E5, E5, what + " side output")
        else:
            assert torch.equal(xs.ref.flat().view(torch.int32), xs.before.view(torch.int32))
        assert torch.equal(x.ref.flat().view(torch.int32), x.before.view(torch.int32))


# --------------------------------------------------------------------------------------
# the B loop of ops.pw_fwd / pw_dw / pw_fwd_tshift
# --------------------------------------------------------------------------------------
def _force_chunks(monkeypatch, ops, views, B, T, V, want=2):
    """PW_MAX_ELEMS such that ``_batch_chunk`` gives ``want`` samples per launch."""
    lim = max(C * v.cstride + T * v.tstride * V + (want - 1) * v.bstride for v, C in views) + 1
    monkeypatch.setattr(ops, "PW_MAX_ELEMS", lim)
    assert ops._batch_chunk(views, B, T, V) == want and B % want


@pytest.mark.parametrize("M,K", [(37, 51), (130, 37), (3, 64)])
def test_batch_chunking_forward_is_bit_identical(monkeypatch, M, K):
    from shiftgcn import ops
    from shiftgcn.ops import PlaneView as PV
    B, T, V = 5, 7, 25
    x = pc.rnd((B, K, T, V), 1).to(DEV)
    w = pc.rnd((M, K), 2, K ** -0.5).to(DEV)
    bias = pc.rnd((M,), 3).to(DEV)
    old = pc.rnd((B, M, T, V), 4).to(DEV)
    rot = 0 if M <= pc.K_SMALL_M else 1
    whole, parts = old.clone(), old.clone()
    ops.pw_fwd(w, False, bias, PV(x, 1, rot), PV(whole, 1, rot), M, K, T, V, relu=True,
               accumulate=True)
    _force_chunks(monkeypatch, ops, [(PV(x), K), (PV(parts), M)], B, T, V)
    ops.pw_fwd(w, False, bias, PV(x, 1, rot), PV(parts, 1, rot), M, K, T, V, relu=True,
               accumulate=True)
    assert torch.equal(whole, parts) and not torch.equal(whole, old)


@pytest.mark.parametrize("case", [(5, 100, 37, 9, 25), (5, 40, 300, 5, 25)], ids=_id)
def test_batch_chunking_tshift_is_bit_identical(monkeypatch, case):
    from shiftgcn import ops
    from shiftgcn.ops import PlaneView as PV
    B, K, M, T, V = case
    h, w, bias, xpos, ypos, scale, shift = _tshift_inputs(*case, seed=3)
    h = h.to(DEV)
    out = []
    for chunked in (False, True):
        if chunked:
            _force_chunks(monkeypatch, ops, [(PV(h), K), (PV(torch.empty(B, M, T, V, device=DEV)), M)],
                          B, T, V)
        y = torch.full((B, M, T, V), float("nan"), device=DEV)
        xs = torch.full_like(h, float("nan"))
        ops.pw_fwd_tshift(w, bias, PV(h), xpos, ypos, _St(scale, shift), PV(y), M, K, T, V,
                          relu=True, x_shifted=xs)
        out.append((y, xs))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[1][0]).all() and torch.isfinite(out[1][1]).all()


@pytest.mark.parametrize("shape", [(5, 64, 64, 5, 25), (5, 129, 128, 5, 25), (5, 64, 3, 17, 25)],
                         ids=_id)
@pytest.mark.parametrize("accumulate", [False, True])
def test_batch_chunking_dw_within_the_bar(monkeypatch, shape, accumulate):
    """Chunks of 2, 2 and 1 samples: the later launches accumulate into the first's result
    (and into the previous contents when the caller accumulates), dbias likewise."""
    from shiftgcn import ops
    from shiftgcn.ops import PlaneView as PV
    B, M, Nc, T, V = shape
    g = pc.rnd((B, M, T, V), 1).to(DEV)
    x = pc.rnd((B, Nc, T, V), 2).to(DEV)
    old_w, old_b = pc.rnd((M, Nc), 3, 3.0).to(DEV), pc.rnd((M,), 4, 3.0).to(DEV)
    dw_ref, db_ref = pr.pw_dw_ref(pr.Plane(g), pr.Plane(x), M, Nc, T, V,
                                  dw_old=old_w if accumulate else None,
                                  dbias_old=old_b if accumulate else None)
    _force_chunks(monkeypatch, ops, [(PV(g), M), (PV(x), Nc)], B, T, V)
    dw, db = old_w.clone(), old_b.clone()
    ops.pw_dw(PV(g), PV(x), dw, M, Nc, T, V, accumulate=accumulate, dbias=db,
              dbias_accumulate=accumulate)
    _check(dw, dw_ref, E5, DW_ATOL, f"chunked pw_dw {_id(shape)} acc{int(accumulate)} dW")
    _check(db, db_ref, E5, DW_ATOL, f"chunked pw_dw {_id(shape)} acc{int(accumulate)} dbias")
