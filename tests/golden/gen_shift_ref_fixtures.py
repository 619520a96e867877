"""Results of the REFERENCE's own temporal-shift kernels at every launch form of the HIP entry
points, for the GPU machine (where the reference tree does not exist).

    python tests/golden/gen_shift_ref_fixtures.py

needs the exact host build of the reference kernels (``oracle/ref_build.py``, made by
``build()`` where the reference tree exists) and writes ``shift_ref_fixtures.npz``. Inputs are
not stored: they come from ``oracle.tshift_cases.fwd_inputs`` / ``bwd_inputs``.

Cases (:func:`cases`): for every value ``tshift_cases.fwd_form`` and ``bwd_form`` return over
``tshift_cases.TABLE``, the first shape that reaches it, at stride 1 and 2, in float32; the
``F64_CASES`` in float64. Every case runs all its position variants
(``stream_cases.positions``: 8 entries over the channels; :data:`SECOND_ROUND`).

Stored per case, stacked over the variants:

* ``out`` (forward, ``fwd_inputs``) and ``gin`` (input gradient, ``bwd_inputs``): the array
  where the input holds at most :data:`SMALL` elements, else ``*_sha256``, the SHA-256 of the
  raw little-endian bytes in C order;
* ``part``: float64 per-plane sums (B, C, 2) = {x, y} of the reference's per-element position
  products (.cu:348-349);
* ``gx`` / ``gy``: the finalized position gradients of ``shift_cuda_backward`` (.cu:501-520,
  ATen's mean / sum as torch-CPU runs them).

The finalized values carry only the sign of a batch mean, so a consumer compares them on the
channels ``stream_cases.gy_unsafe`` keeps. :func:`check_signs` asserts here, on the CPU, that
no case drops more than one channel in eight and that every case keeps at least two channels
of each sign of gy (the empty case, H // stride == 0, has no product and is exempt), and that
on the kept channels the reference's values equal the constraint of the float64 batch mean.

:func:`compute` takes the kernels as an argument: ``tests/test_oracle_shift_ref.py`` runs it
with ``oracle.shift_oracle`` (must reproduce the committed file, always) and with the compiled
reference (must too, where the library exists).
"""
from __future__ import annotations

import functools
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import shift_oracle as so  # noqa: E402
from oracle import stream_cases as sc  # noqa: E402
from oracle import tshift_cases as tc  # noqa: E402

FILE = "shift_ref_fixtures.npz"
SMALL = 2048          # input elements up to which out / gin are stored whole
DTYPES = {"f32": np.float32, "f64": np.float64}


def cases():
    """[(dtype name, shape, stride, (fwd form, bwd form))]: see the module docstring."""
    out = []
    for stride in (1, 2):
        seen_f, seen_b = set(), set()
        for shape in tc.TABLE:
            H, W = shape[2], shape[3]
            ff, bf = tc.fwd_form(H, W, stride), tc.bwd_form(H, W, stride)
            if ff not in seen_f or bf not in seen_b:
                out.append(("f32", shape, stride, (ff, bf)))
            seen_f.add(ff)
            seen_b.add(bf)
    for shape, stride in tc.F64_CASES:
        H, W = shape[2], shape[3]
        out.append(("f64", shape, stride, (tc.fwd_form(H, W, stride),
                                           tc.bwd_form(H, W, stride))))
    return out


# Cases whose first round of variants keeps a single channel with a negative gy (6 positive, 1
# negative, 1 dead with the table's seeds): they run a second round, the same position cycle
# on the next seeds, which brings them to two or more of each sign (check_signs).
SECOND_ROUND = {"f32_2x2x9x70_s1", "f32_2x2x40x70_s1"}


def n_variants(dtype, shape, stride):
    n = tc.n_variants(shape[1])
    return 2 * n if case_key(dtype, shape, stride) in SECOND_ROUND else n


def case_key(dtype, shape, stride):
    return f"{dtype}_" + "x".join(map(str, shape)) + f"_s{stride}"


@functools.lru_cache(maxsize=None)
def _raw_inputs(shape, stride, variant):
    """The float32 tensors of one variant, generated once for both precisions (read-only)."""
    f = tc.fwd_inputs(shape, variant, stride)
    k = tc.bwd_inputs(shape, variant, stride)
    raw = dict(inp_f=f[0].numpy(), inp_b=k["inp"].numpy(), gout=k["gout"].numpy(),
               xpos=k["xpos"].numpy(), ypos=k["ypos"].numpy())
    for a in raw.values():
        a.setflags(write=False)
    return raw


def case_inputs(dtype, shape, stride, variant):
    """numpy inputs of one variant: dict(inp_f, inp_b, gout, xpos, ypos (raw), ye (effective:
    the add in the case's precision, as ShiftFunction and the float64 entry point do))."""
    dt = DTYPES[dtype]
    k = {n: a.astype(dt) for n, a in _raw_inputs(tuple(shape), stride, variant).items()}
    k["ye"] = so.effective_ypos(k["ypos"], stride)
    return k


def digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.astype(a.dtype.newbyteorder("<")).tobytes()).digest(),
                         np.uint8).copy()


def is_small(shape):
    return int(np.prod(shape)) <= SMALL


class OracleKernels:
    """``oracle.shift_oracle`` behind the call surface :func:`compute` uses."""

    forward = staticmethod(so.shift_forward)

    @staticmethod
    def backward(gout, inp, xpos, ye, stride):
        gin, gx, gy = so.shift_backward(gout, inp, xpos, ye, stride)
        gxb, gyb = so.shift_position_backward(inp, gout, xpos, ye, stride)
        return gin, gx, gy, gxb, gyb


def reference_kernels():
    from oracle import shift_ref
    shift_ref.shift_cuda_module()       # raises where the library is not built
    return shift_ref


def compute(kernels, only=None):
    """{key: array} of every case (or of the case keys in ``only``) through ``kernels``."""
    out = {}
    for dtype, shape, stride, _ in cases():
        key = case_key(dtype, shape, stride)
        if only is not None and key not in only:
            continue
        rec = {n: [] for n in ("out", "gin", "part", "gx", "gy")}
        for v in range(n_variants(dtype, shape, stride)):
            k = case_inputs(dtype, shape, stride, v)
            rec["out"].append(kernels.forward(k["inp_f"], k["xpos"], k["ye"], stride))
            gin, gx, gy, gxb, gyb = kernels.backward(k["gout"], k["inp_b"], k["xpos"], k["ye"],
                                                     stride)
            rec["gin"].append(gin)
            rec["part"].append(np.stack((gxb.astype(np.float64).sum((2, 3)),
                                         gyb.astype(np.float64).sum((2, 3))), -1))
            rec["gx"].append(gx)
            rec["gy"].append(gy)
        for n in ("out", "gin"):
            if is_small(shape):
                out[f"{key}_{n}"] = np.stack(rec[n])
            else:
                out[f"{key}_{n}_sha256"] = np.stack([digest(a) for a in rec[n]])
        for n in ("part", "gx", "gy"):
            out[f"{key}_{n}"] = np.stack(rec[n])
    return out


def kept(part):
    """Channels (C,) bool of one variant on which the finalized gx / gy are sign-robust."""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(part))
    return (~sc.gy_unsafe(p, p.mean(0))).numpy()


def check_signs(fx):
    for dtype, shape, stride, _ in cases():
        key = case_key(dtype, shape, stride)
        part, gx, gy = fx[f"{key}_part"], fx[f"{key}_gx"], fx[f"{key}_gy"]
        nv, C = gy.shape
        keep = np.stack([kept(part[v]) for v in range(nv)])
        assert (~keep).sum() * 8 <= nv * C, (key, "drops more than one channel in eight")
        dt = DTYPES[dtype]
        for v in range(nv):
            mean = part[v].mean(0).astype(dt)
            wx, wy = so.apply_shift_constraint(mean[:, 0], mean[:, 1])
            assert np.array_equal(gy[v][keep[v]], wy[keep[v]]), (key, v, gy[v], wy)
            assert np.array_equal(gx[v][keep[v]], wx[keep[v]]), (key, v, gx[v], wx)
        if shape[2] // stride == 0:
            assert np.all(gy == dt(0.0001)), key
            continue
        g = gy[keep]
        assert (g > 0.001).sum() >= 2 and (g < 0).sum() >= 2, (key, "signs of gy", gy)


def load():
    return np.load(os.path.join(HERE, FILE), allow_pickle=False)


def main():
    fx = compute(reference_kernels())
    check_signs(fx)
    path = os.path.join(HERE, FILE)
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes,", len(fx), "arrays,", len(cases()), "cases")


if __name__ == "__main__":
    main()
