"""The plain temporal-shift entry points against results of the REFERENCE's own kernel code.

``tests/golden/shift_ref_fixtures.npz`` was written by ``gen_shift_ref_fixtures.py`` from the
reference's kernel templates compiled for the host (``oracle/ref_build.py``); it holds, for
the first ``tshift_cases.TABLE`` shape at every launch form of ``sgcn_tshift_fwd`` and
``sgcn_tshift_bwd`` (pad, LDS and global forward; ra at 256 and 512 threads; s2 with and
without the joint-aligned walk; the global backward in one and several passes) at stride 1
and 2, and for the float64 cases, the reference's output and input gradient (whole, or as a
SHA-256 of the bytes), float64 plane sums of its position products and its finalized
gx / gy. Nothing here reads the reference tree.

Bit for bit, inside test_gpu_tshift_ref's sentinel guard: ``ops.tshift_fwd`` without affine
and statistics, the input gradient of the plain ``ops.tshift_bwd``, ``sgcn_tshift_fwd_f64``
and ``sgcn_tshift_bwd_f64``. The HIP per-plane position partials hold to the fixture's
float64 sums at the bar of ``test_gpu_tshift_ref._check_pos`` (SUM = 1e-5 of the largest sum
of each kind), and ``ShiftFunction``'s finalized gx / gy equal the reference's exactly on the
channels ``stream_cases.gy_unsafe`` keeps (the generator asserts, on the CPU, that at most
one channel in eight is dropped and two of each sign stay).

On a mismatch with a digest the message names the case and the first element that differs
from ``oracle.shift_oracle``, which ``tests/test_oracle_shift_ref.py`` holds equal to the
fixture without a GPU.
"""
import numpy as np
import pytest
import torch

import gen_shift_ref_fixtures as gr
from oracle import shift_oracle as so
from test_gpu_stream_ref import _check_sums
from test_gpu_tshift_ref import DEV, _dev, _guard

pytestmark = pytest.mark.gpu

CASES = gr.cases()


def _id(c):
    return gr.case_key(*c[:3])


@pytest.fixture(scope="module")
def fx(golden):
    return golden(gr.FILE)


def _expect(fx, key, name, v, got, oracle, what):
    """``got`` (a device tensor) against the fixture's array or digest of variant ``v``."""
    got = got.cpu().numpy()
    if f"{key}_{name}" in fx.files:
        want = fx[f"{key}_{name}"][v]
        assert got.dtype == want.dtype and got.shape == want.shape, what
        ok = got.tobytes() == want.tobytes()
    else:
        ok = gr.digest(got).tobytes() == fx[f"{key}_{name}_sha256"][v].tobytes()
        want = None
    if ok:
        return
    want = oracle() if want is None else want
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    ne = np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)
    i = tuple(int(j) for j in np.argwhere(ne)[0]) if ne.any() else None
    raise AssertionError(
        f"{what}: differs from the reference kernels' result; {int(ne.sum())} of {ne.size} "
        f"elements differ from oracle.shift_oracle, first at {i}: got "
        f"{got[i] if i else None!r}, oracle {want[i] if i else None!r}")


def _kept(fx, key, v):
    return torch.from_numpy(gr.kept(fx[f"{key}_part"][v]))


def _equal_kept(got, fx, key, name, v, keep, what):
    want = torch.from_numpy(fx[f"{key}_{name}"][v])
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(got[keep].view(torch.int64 if got.dtype == torch.float64 else torch.int32),
                       want[keep].view(torch.int64 if got.dtype == torch.float64
                                       else torch.int32)), (what, got, want, keep)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "f32"], ids=_id)
def test_refpin_f32(fx, case):
    from shiftgcn import ShiftFunction, ops
    dtype, shape, stride, forms = case
    B, C, H, W = shape
    key = gr.case_key(dtype, shape, stride)
    for v in range(gr.n_variants(dtype, shape, stride)):
        k = gr.case_inputs(dtype, shape, stride, v)
        d = {n: _dev(torch.from_numpy(a)) for n, a in k.items()}
        tag = f"{key} v{v} {forms}"
        with _guard(tag + " fwd"):
            out = ops.tshift_fwd(d["inp_f"], d["xpos"], d["ypos"], stride)
        assert out.shape == (B, C, H // stride, W)
        _expect(fx, key, "out", v, out,
                lambda: so.shift_forward(k["inp_f"], k["xpos"], k["ye"], stride), tag + " out")
        with _guard(tag + " bwd"):
            gin, pp, none = ops.tshift_bwd(d["gout"], d["inp_b"], d["xpos"], d["ypos"], stride,
                                           defer_pos=True)
        assert none is None
        _expect(fx, key, "gin", v, gin,
                lambda: so.shift_bottom_backward(k["gout"], k["xpos"], k["ye"], H, stride),
                tag + " gin")
        _check_sums(pp.ws[:2 * B * C], torch.from_numpy(fx[f"{key}_part"][v]).to(DEV),
                    tag + " pos_part")
        # ShiftFunction: the finalized position gradients
        x = d["inp_b"].clone().requires_grad_(True)
        xp = d["xpos"].clone().requires_grad_(True)
        yp = d["ypos"].clone().requires_grad_(True)
        y = ShiftFunction.apply(x, xp, yp, stride)
        y.backward(d["gout"])
        assert torch.equal(x.grad, gin), tag + ": ShiftFunction's input gradient"
        keep = _kept(fx, key, v)
        _equal_kept(yp.grad, fx, key, "gy", v, keep, tag + " gy")
        _equal_kept(xp.grad, fx, key, "gx", v, keep, tag + " gx")
        for n, t in d.items():      # no input was written
            assert t.cpu().numpy().tobytes() == k[n].tobytes(), (tag, n)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "f64"], ids=_id)
def test_refpin_f64(fx, case):
    from shiftgcn import ops
    dtype, shape, stride, forms = case
    B, C, H, W = shape
    key = gr.case_key(dtype, shape, stride)
    for v in range(gr.n_variants(dtype, shape, stride)):
        k = gr.case_inputs(dtype, shape, stride, v)
        d = {n: _dev(torch.from_numpy(a)) for n, a in k.items()}
        tag = f"{key} v{v}"
        with _guard(tag + " fwd"):
            out = ops.tshift_fwd(d["inp_f"], d["xpos"], d["ypos"], stride)
        assert out.dtype == torch.float64
        _expect(fx, key, "out", v, out,
                lambda: so.shift_forward(k["inp_f"], k["xpos"], k["ye"], stride), tag + " out")
        with _guard(tag + " bwd"):
            gin, gx, gy = ops.tshift_bwd(d["gout"], d["inp_b"], d["xpos"], d["ypos"], stride)
        assert gin.dtype == torch.float64
        _expect(fx, key, "gin", v, gin,
                lambda: so.shift_bottom_backward(k["gout"], k["xpos"], k["ye"], H, stride),
                tag + " gin")
        keep = _kept(fx, key, v)
        _equal_kept(gy, fx, key, "gy", v, keep, tag + " gy")
        _equal_kept(gx, fx, key, "gx", v, keep, tag + " gx")
