"""Pin the temporal-shift oracle to the reference's own kernel code (CPU; no GPU needed).

``oracle/ref_build.py`` compiles the five kernel templates of the reference's
``shift_cuda_kernel.cu`` (.cu:11-395) for the host; ``oracle/shift_ref.py`` runs them. Here
``oracle.shift_oracle`` (and ``oracle.shift_loops`` on the small planes) is held equal to the
exact build BIT FOR BIT, compared through the integer view of the floats so that the sign of
a zero and the payload of a NaN count:

* forward (stride 1, 2, 3), both bottom backwards, both per-element position products and the
  constraint, in float32 and float64;
* every plane H 0..12 x W 1..9 with 16 channels per position set, and every plane of
  ``tshift_cases.TABLE`` under every ``stream_cases.positions`` variant;
* positions (:func:`position_pool`): 0, +-1e-8, positive and negative integers, half-integers,
  other fractions, |y| > H, |x| > W, |pos| up to 2^20; in float64 also doubles that round to a
  float across an integer (``1 - 1e-12``, ``-1e-50``): ``floorf((float)x)`` then leaves
  ``dx`` negative or >= 1, which ``tshift64.hip`` copies on purpose;
* inputs with +-inf, NaN (with a payload), -0.0 and denormals.

Range: |pos| < 2^31 - H * stride throughout. Beyond it the C++ float -> int conversion and the
index sums are undefined, and the host build no longer stands in for the CUDA one
(``tests/shift_ref_sanitize_main.cpp`` runs this range under the address and
undefined-behaviour sanitizers, by hand).

The contracted build (``-ffp-contract=fast -mfma``) is held within the project's 1e-5 bar of
the oracle's ``contract=True`` variant and of the exact result; never bit-equal, compilers
choose their own contractions.

Skips: where the reference tree exists and the library does not, these tests FAIL (run
``build()``). Elsewhere the library-dependent ones skip;
``test_oracle_reproduces_committed_fixture`` never does.
"""
import numpy as np
import pytest

import gen_fixtures as gf
import gen_shift_ref_fixtures as gr
from oracle import ref_build as rb
from oracle import shift_loops as sl
from oracle import shift_oracle as so
from oracle import shift_ref as sr
from oracle import tshift_cases as tc

F32, F64 = np.float32, np.float64
C_SWEEP = 16
BAR = 1e-5                  # DESIGN §Parity bars: max |a - b| <= 1e-5 x max |reference|


def _need_lib(contracted=False):
    if sr.available(contracted):
        return
    import os
    built = os.path.isfile(os.path.join(rb.OUT_DIR, rb.LIB_FMA if contracted else rb.LIB_EXACT))
    if contracted and built:
        pytest.skip("this CPU has no FMA: the contracted build cannot run")
    if rb.have_reference():
        pytest.fail("the reference tree is here but its kernels are not built: run build()")
    pytest.skip("no reference tree and no prebuilt reference-kernel library")


@pytest.fixture(scope="module")
def ref():
    _need_lib()
    return sr


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape,
                                                                 want.dtype, want.shape)
    ne = _bits(got) != _bits(want)
    if ne.any():
        i = tuple(int(j) for j in np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {i}: "
                             f"oracle {got[i]!r} ({_bits(got)[i]:#x}) reference {want[i]!r} "
                             f"({_bits(want)[i]:#x})")


# ----------------------------------------------------------------------------------------
# positions
# ----------------------------------------------------------------------------------------
def position_pool(H, W, dtype):
    """[(x, y)]: every class of the module docstring on some entry, in x and in y."""
    big = float(2 ** 20)
    xs = [0.0, 1e-8, -1e-8, 1.0, -2.0, 3.0, 0.5, -1.5, 0.3, -0.7, W + 1.25, -(W + 2.5),
          big, -big + 0.5, 2.5, -0.25]
    ys = [0.0, -1e-8, 1e-8, -1.0, 2.0, -4.0, -0.5, 3.5, 1.3, -2.75, -(H + 1.5), H + 2.25,
          -big, big - 0.5, 5.0, 0.75]
    pool = list(zip(xs, ys))
    # the same values crossed, so that e.g. an integer y meets a fractional x and back
    pool += list(zip(xs, ys[5:] + ys[:5]))
    if dtype == F64:
        edge = [1.0 - 1e-12, -1e-50, -1.0 - 1e-12, 1e-50, 3.0 - 1e-13, -(2.0 + 1e-12)]
        pool += [(e, ys[i]) for i, e in enumerate(edge)]
        pool += [(xs[i + 6], e) for i, e in enumerate(edge)]
    while len(pool) % C_SWEEP:
        pool.append(pool[len(pool) % 7])
    return pool


def _sets(H, W, dtype):
    pool = position_pool(H, W, dtype)
    for s in range(0, len(pool), C_SWEEP):
        chunk = pool[s:s + C_SWEEP]
        yield (np.array([p[0] for p in chunk], dtype), np.array([p[1] for p in chunk], dtype))


def test_position_pool_holds_every_class():
    for dtype in (F32, F64):
        H, W = 7, 5
        pool = np.array(position_pool(H, W, dtype), dtype)
        limit = 2.0 ** 31 - 12 * 3
        assert np.abs(pool).max() < limit and np.abs(pool).max() >= 2 ** 20
        for axis, size in ((0, W), (1, H)):
            v = pool[:, axis]
            fr = v - np.floor(v)
            assert (v == 0).any() and (v == dtype(1e-8)).any() and (v == dtype(-1e-8)).any()
            assert ((fr == 0) & (v > 0)).any() and ((fr == 0) & (v < 0)).any()
            assert ((fr == 0.5) & (v > 0)).any() and ((fr == 0.5) & (v < 0)).any()
            assert (v > size).any() and (v < -size).any()
            if dtype == F64:
                # doubles whose float rounding crosses an integer: floorf((float)v) != floor(v)
                assert (np.floor(v.astype(F32)).astype(F64) != np.floor(v)).sum() >= 4


# ----------------------------------------------------------------------------------------
# a. the sweep, bit for bit
# ----------------------------------------------------------------------------------------
def _compare_plane(ref, x, g_by_stride, xp, yp, strides, what, loops=False):
    H = x.shape[2]
    for stride in strides:
        tag = f"{what} s{stride}"
        out = so.shift_forward(x, xp, yp, stride)
        _same(out, ref.forward(x, xp, yp, stride), tag + " forward")
        if loops:
            _same(sl.forward(x, xp, yp, stride), out, tag + " loops forward")
        if stride > 2:
            continue
        g = g_by_stride[stride]
        gin = so.shift_bottom_backward(g, xp, yp, H, stride)
        _same(gin, ref.bottom_backward(g, xp, yp, H, stride), tag + " bottom backward")
        a = so.shift_position_backward(x, g, xp, yp, stride)
        b = ref.position_backward(x, g, xp, yp, stride)
        _same(a[0], b[0], tag + " position product x")
        _same(a[1], b[1], tag + " position product y")
        if loops:
            _same(sl.bottom_backward(g, xp, yp, H, stride), gin, tag + " loops bottom backward")
            c = sl.position_backward(x, g, xp, yp, stride)
            _same(c[0], a[0], tag + " loops product x")
            _same(c[1], a[1], tag + " loops product y")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_sweep_small_planes(ref, dtype):
    """H 0..12 x W 1..9 exhaustively, B = 2, 16 channels per position set."""
    rng = np.random.default_rng(20 if dtype == F32 else 21)
    B = 2
    for H in range(13):
        for W in range(1, 10):
            x = rng.standard_normal((B, C_SWEEP, H, W)).astype(dtype)
            g = {s: rng.standard_normal((B, C_SWEEP, H // s, W)).astype(dtype) for s in (1, 2)}
            for n, (xp, yp) in enumerate(_sets(H, W, dtype)):
                _compare_plane(ref, x, g, xp, yp, (1, 2, 3), f"H{H} W{W} set{n}")


def test_sweep_scalar_loops(ref):
    """The second restatement (float32, one Python iteration per CUDA thread) on the smallest
    planes, against the oracle, which the same call holds equal to the reference."""
    rng = np.random.default_rng(22)
    for H, W in ((0, 2), (1, 1), (2, 3), (5, 2), (4, 3)):
        x = rng.standard_normal((1, C_SWEEP, H, W)).astype(F32)
        g = {s: rng.standard_normal((1, C_SWEEP, H // s, W)).astype(F32) for s in (1, 2)}
        for n, (xp, yp) in enumerate(_sets(H, W, F32)):
            _compare_plane(ref, x, g, xp, yp, (1, 2, 3), f"H{H} W{W} set{n}", loops=True)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_sweep_table_planes(ref, dtype):
    """Every plane of tshift_cases.TABLE (+ the stride-3 forward) under every position
    variant, with the effective ypos the entry points form."""
    dt = gr.DTYPES[dtype]
    for shape, stride in tc.FWD_CASES:
        for v in range(tc.n_variants(shape[1])):
            k = gr.case_inputs(dtype, shape, stride, v)
            tag = f"{gr.case_key(dtype, shape, stride)} v{v}"
            assert k["inp_f"].dtype == dt
            _same(so.shift_forward(k["inp_f"], k["xpos"], k["ye"], stride),
                  ref.forward(k["inp_f"], k["xpos"], k["ye"], stride), tag + " forward")
            if stride > 2:
                continue
            _compare_plane(ref, k["inp_b"], {stride: k["gout"]}, k["xpos"], k["ye"], (stride,),
                           tag)


def _special(shape, dtype, kind, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(dtype)
    flat = a.reshape(-1)
    idx = rng.permutation(flat.size)[:max(4, flat.size // 5)]
    tiny = np.finfo(dtype).tiny
    if kind == "inf":
        flat[idx[::2]], flat[idx[1::2]] = np.inf, -np.inf
    elif kind == "nan":
        nan = np.array([0x7FC12345], np.uint32).view(F32)[0] if dtype == F32 else \
            np.array([0x7FF8000012345678], np.uint64).view(F64)[0]
        flat[idx] = nan
    elif kind == "negzero":
        flat[idx[::2]], flat[idx[1::2]] = -0.0, 0.0
    elif kind == "denormal":
        flat[idx] = (rng.standard_normal(idx.size) * tiny / 8).astype(dtype)
        assert (np.abs(flat[idx]) < tiny).all() and (flat[idx] != 0).any()
    return a


@pytest.mark.parametrize("kind", ["inf", "nan", "negzero", "denormal"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_sweep_special_inputs(ref, dtype, kind):
    """One case each with +-inf, NaN (a payload of its own), +-0.0 and denormals among the
    inputs and the gradient; NaN results are compared by sign and payload like any other."""
    H, W, B = 9, 7, 2
    x = _special((B, C_SWEEP, H, W), dtype, kind, 30)
    g = {s: _special((B, C_SWEEP, H // s, W), dtype, kind, 31 + s) for s in (1, 2)}
    with np.errstate(invalid="ignore"):
        for n, (xp, yp) in enumerate(_sets(H, W, dtype)):
            _compare_plane(ref, x, g, xp, yp, (1, 2, 3), f"{kind} set{n}")
        out = ref.forward(x, *next(_sets(H, W, dtype)), 1)
    assert np.isnan(out).any() == (kind in ("inf", "nan"))


def _constraint_values(dtype):
    rng = np.random.default_rng(40)
    tiny = [0.0, -0.0, 1e-30, -1e-30, 1e-20, -1e-20, 1e-23, 3e-23, 1e30, -1e30, 1.0, -1.0,
            3.7, -0.01, 0.0001, np.inf, -np.inf, 2.0 ** -75, -(2.0 ** -74), 1e-38, 1e-45, -1e-45]
    if dtype == F64:
        tiny += [1e-160, -1e-162, 1e-200, -1e-170, 1e160, -1e155, 5e-324, -5e-324]
    gy = np.array(tiny, dtype)
    gy = np.concatenate([gy, rng.standard_normal(64 - gy.size).astype(dtype)
                         * dtype(10.0) ** rng.integers(-6, 6, 64 - gy.size).astype(dtype)])
    gx = rng.standard_normal(64).astype(dtype)
    gx[::7] = [0.0, -0.0, np.inf, 1e-30, -1e30, 1.0, -2.0, 5.0, 0.0, -0.0][:len(gx[::7])]
    return gx, gy.astype(dtype)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_constraint(ref, dtype):
    """applyShiftConstraint on 64 values: +-0, values whose square underflows to 0 or to a
    denormal or overflows, +-inf (inf / inf: a fresh NaN on both sides), ordinary ones."""
    gx, gy = _constraint_values(dtype)
    with np.errstate(all="ignore"):
        assert gy.size == 64 and (gy == 0).sum() >= 2 and (gy * gy == 0).sum() > (gy == 0).sum()
        a = so.apply_shift_constraint(gx, gy)
    b = ref.constraint(gx, gy)
    _same(a[0], b[0], "constraint gx")
    _same(a[1], b[1], "constraint gy")
    # ... and composed as shift_cuda_backward composes it, on a plane whose sums are robust
    k = gr.case_inputs("f32" if dtype == F32 else "f64", (2, 5, 7, 25), 1, 0)
    gin, rgx, rgy, _, _ = ref.backward(k["gout"], k["inp_b"], k["xpos"], k["ye"], 1)
    ogin, ogx, ogy = so.shift_backward(k["gout"], k["inp_b"], k["xpos"], k["ye"], 1)
    _same(ogin, gin, "backward gin")
    _same(ogx, rgx, "backward gx")
    _same(ogy, rgy, "backward gy")


# ----------------------------------------------------------------------------------------
# b. the committed fixture
# ----------------------------------------------------------------------------------------
def _assert_fixture_equal(got, fx, who):
    assert sorted(got) == sorted(fx.files), (who, set(got) ^ set(fx.files))
    for key in fx.files:
        a, b = got[key], fx[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (who, key, a.dtype, a.shape, b.dtype,
                                                           b.shape)
        if key.endswith(("_gx", "_gy")):
            continue
        assert a.tobytes() == b.tobytes(), f"{who}: {key} differs from the committed fixture"


def test_oracle_reproduces_committed_fixture(golden):
    """Always runs, needs no library: oracle.shift_oracle reproduces every array, digest and
    plane sum of the reference-kernel fixture, and its finalized gx / gy on every channel the
    fixture's consumers compare (all but the sign-fragile ones, gy_unsafe)."""
    fx = golden(gr.FILE)
    gr.check_signs(fx)
    got = gr.compute(gr.OracleKernels)
    _assert_fixture_equal(got, fx, "oracle")
    for dtype, shape, stride, _ in gr.cases():
        key = gr.case_key(dtype, shape, stride)
        for v in range(gr.n_variants(dtype, shape, stride)):
            keep = gr.kept(fx[f"{key}_part"][v])
            for n in ("gx", "gy"):
                _same(got[f"{key}_{n}"][v][keep], fx[f"{key}_{n}"][v][keep], f"{key} v{v} {n}")


def test_fixture_size_and_cases(golden):
    import os
    here = os.path.dirname(gr.__file__)
    assert os.path.getsize(os.path.join(here, gr.FILE)) <= \
        os.path.getsize(os.path.join(here, "shift_fixtures.npz"))
    forms_f = {c[3][0] for c in gr.cases() if c[0] == "f32"}
    forms_b = {c[3][1] for c in gr.cases() if c[0] == "f32"}
    for stride in (1, 2):
        for shape in tc.TABLE:
            assert tc.fwd_form(shape[2], shape[3], stride) in forms_f
            assert tc.bwd_form(shape[2], shape[3], stride) in forms_b
    kinds = {f[0] for f in forms_f if f != "empty"}, {f[0] for f in forms_b}
    assert kinds == ({"pad", "lds", "global"}, {"ra", "s2", "global"})
    assert {f[1] for f in forms_b if f[0] == "ra"} == {256, 512}
    assert {f[2] for f in forms_b if f[0] == "s2"} == {True, False}
    assert {f[3] for f in forms_b if f[0] == "global"} == {True, False}


def test_fixture_is_fresh(ref, golden):
    """Regenerating through the compiled reference equals the committed file, gx / gy too."""
    fx = golden(gr.FILE)
    got = gr.compute(gr.reference_kernels())
    _assert_fixture_equal(got, fx, "reference")
    for key in fx.files:
        assert got[key].tobytes() == fx[key].tobytes(), key


# ----------------------------------------------------------------------------------------
# c. the contracted build
# ----------------------------------------------------------------------------------------
def _rel(a, b, scale):
    return float(np.abs(a.astype(F64) - b.astype(F64)).max()) / float(np.abs(scale).max())


@pytest.mark.parametrize("stride", [1, 2])
def test_contracted_build_within_bar(stride):
    """-ffp-contract=fast -mfma of the reference text, the oracle's contract=True variant and
    the uncontracted result: pairwise within 1e-5 of the result's largest value."""
    _need_lib()
    _need_lib(contracted=True)
    rng = np.random.default_rng(50 + stride)
    B, C, H, W = 2, C_SWEEP, 40, 25
    x = rng.standard_normal((B, C, H, W)).astype(F32)
    g = rng.standard_normal((B, C, H // stride, W)).astype(F32)
    worst = 0.0
    for xp, yp in _sets(H, W, F32):
        yp = so.effective_ypos(yp, stride)
        exact = [sr.forward(x, xp, yp, stride), sr.bottom_backward(g, xp, yp, H, stride),
                 *sr.position_backward(x, g, xp, yp, stride)]
        fma = [sr.forward(x, xp, yp, stride, True), sr.bottom_backward(g, xp, yp, H, stride, True),
               *sr.position_backward(x, g, xp, yp, stride, True)]
        orc = [so.shift_forward(x, xp, yp, stride, True),
               so.shift_bottom_backward(g, xp, yp, H, stride, True),
               *so.shift_position_backward(x, g, xp, yp, stride, True)]
        for e, f, o, what in zip(exact, fma, orc, ("forward", "gin", "product x", "product y")):
            figs = (_rel(f, o, e), _rel(f, e, e), _rel(o, e, e))
            print(f"s{stride} {what}: fma build vs oracle(contract) {figs[0]:.2e}, fma build vs "
                  f"exact {figs[1]:.2e}, oracle(contract) vs exact {figs[2]:.2e}")
            worst = max(worst, *figs)
            assert max(figs) <= BAR, (what, figs)
    print(f"s{stride}: worst {worst:.3e}")


# ----------------------------------------------------------------------------------------
# d. the glue fixtures through the reference kernels
# ----------------------------------------------------------------------------------------
def test_glue_fixture_through_reference_kernels(ref, golden):
    """The reference's ShiftFunction (shift.py) over the compiled reference kernels reproduces
    the ``shift_*`` arrays of the committed shift_fixtures.npz, which were generated with the
    restatement behind ``shift_cuda``."""
    if not rb.have_reference():
        pytest.skip("the reference's Python glue is not on this machine")
    fx = golden("shift_fixtures.npz")
    _, ref_shift = gf._import_reference()
    prev = gf.use_kernels("reference")
    try:
        out = {}
        gf.gen_shift(ref_shift, out)
    finally:
        gf.use_kernels(prev)
    assert sorted(out) == sorted(k for k in fx.files if k.startswith("shift_s"))
    for key, a in out.items():
        _same(a, fx[key], key)
