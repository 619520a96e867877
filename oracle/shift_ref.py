"""ctypes loader of the reference temporal-shift kernels compiled for the host by
``oracle/ref_build.py`` (TEST INFRASTRUCTURE ONLY).

:func:`load` returns ``None`` where the library is absent. The numpy wrappers run the
reference's own kernel bodies (.cu:11-395) over one 1-D grid each; :func:`backward` composes
them as ``shift_cuda_backward`` does (.cu:433-523), with ATen's ``mean(0)``, ``sum(2)``,
``sum(1)`` on torch-CPU tensors; :func:`shift_cuda_module` carries the reference binding's
``forward`` / ``backward`` signature on CPU tensors for ``tests/golden/gen_fixtures.py``.

What stays restated: the allocation and launch arithmetic of .cu:405-523 (the driver in
``ref_build.py``), the reduction order of CUDA's ``at::mean`` / ``at::sum`` (torch-CPU's
order here), and nvcc's own choice of contractions.

Range: the host build stands in for the CUDA one while |pos| < 2^31 - H * stride. Beyond it
the C++ float -> int conversion and the index sums overflow (undefined behaviour on the
host, saturation on the device).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import ref_build as rb

_LIBS: dict = {}
_SUF = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}


def _cpu_has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("flags"):
                    return " fma " in ln + " "
    except OSError:
        pass
    return False


class _Lib:
    def __init__(self, path):
        self.path = path
        self.dll = ctypes.CDLL(path)
        p, i = ctypes.c_void_p, ctypes.c_int
        for suf in ("f32", "f64"):
            for name, args in (("forward", [p] * 4 + [i] * 5), ("bottom_s1", [p] * 4 + [i] * 4),
                               ("bottom_s2", [p] * 4 + [i] * 4), ("position", [p] * 6 + [i] * 5),
                               ("constraint", [p, p, i])):
                fn = getattr(self.dll, f"ref_{name}_{suf}")
                fn.argtypes, fn.restype = args, None

    def fn(self, name, dtype):
        return getattr(self.dll, f"ref_{name}_{_SUF[np.dtype(dtype)]}")


def load(contracted: bool = False):
    """The exact (``-ffp-contract=off``) or the contracted (``-ffp-contract=fast -mfma``) build,
    or None where it has not been built (or, for the contracted one, the CPU has no FMA)."""
    key = bool(contracted)
    if key not in _LIBS:
        path = os.path.join(rb.OUT_DIR, rb.LIB_FMA if contracted else rb.LIB_EXACT)
        ok = os.path.isfile(path) and (not contracted or _cpu_has_fma())
        _LIBS[key] = _Lib(path) if ok else None
    return _LIBS[key]


def available(contracted: bool = False) -> bool:
    return load(contracted) is not None


def _need(contracted):
    lib = load(contracted)
    if lib is None:
        raise RuntimeError("the reference-kernel library is not built (oracle/ref_build.py)")
    return lib


def _arr(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dtype(a):
    dt = np.asarray(a).dtype
    if dt not in _SUF:
        raise TypeError(f"float32 or float64, not {dt}")
    return dt


def forward(inp, xpos, ypos, stride, contracted=False):
    """``shift_cuda_forward_kernel`` launched as .cu:405-431 (``ypos`` the effective value)."""
    lib, dt = _need(contracted), _dtype(inp)
    inp, xp, yp = _arr(inp, dt), _arr(xpos, dt), _arr(ypos, dt)
    B, C, H, W = inp.shape
    assert xp.shape == yp.shape == (C,) and stride >= 1
    out = np.zeros((B, C, H // stride, W), dt)                     # at::zeros, .cu:408
    lib.fn("forward", dt)(_ptr(inp), _ptr(out), _ptr(xp), _ptr(yp), B, C, H, W, stride)
    return out


def bottom_backward(gout, xpos, ypos, H, stride, contracted=False):
    """``Shift_Bottom_Backward_Stride1`` (stride 1) / ``Shift_Bottom_Backward`` (any other
    stride: .cu:448-475; the kernel itself hard-codes 2)."""
    lib, dt = _need(contracted), _dtype(gout)
    gout, xp, yp = _arr(gout, dt), _arr(xpos, dt), _arr(ypos, dt)
    B, C, Ht, W = gout.shape
    assert xp.shape == yp.shape == (C,)
    assert Ht == (H if stride == 1 else H // 2), "grad_output does not fit the bottom plane"
    gin = np.zeros((B, C, H, W), dt)                               # at::zeros_like, .cu:440
    lib.fn("bottom_s1" if stride == 1 else "bottom_s2", dt)(
        _ptr(gout), _ptr(gin), _ptr(xp), _ptr(yp), B, C, H, W)
    return gin


def position_backward(inp, gout, xpos, ypos, stride, contracted=False):
    """``Shift_Position_Backward``: the two (B, C, H // stride, W) product tensors."""
    lib, dt = _need(contracted), _dtype(inp)
    inp, gout, xp, yp = _arr(inp, dt), _arr(gout, dt), _arr(xpos, dt), _arr(ypos, dt)
    B, C, H, W = inp.shape
    assert gout.shape == (B, C, H // stride, W) and xp.shape == yp.shape == (C,)
    gxb, gyb = np.zeros(gout.shape, dt), np.zeros(gout.shape, dt)  # at::zeros, .cu:480-481
    lib.fn("position", dt)(_ptr(inp), _ptr(gout), _ptr(xp), _ptr(yp), _ptr(gxb), _ptr(gyb),
                           B, C, H, W, stride)
    return gxb, gyb


def constraint(gx, gy, contracted=False):
    """``applyShiftConstraint`` on copies of the two (C,) vectors."""
    lib, dt = _need(contracted), _dtype(gy)
    gx, gy = _arr(gx, dt).copy(), _arr(gy, dt).copy()
    assert gx.shape == gy.shape and gx.ndim == 1
    lib.fn("constraint", dt)(_ptr(gx), _ptr(gy), gx.shape[0])
    return gx, gy


def backward(gout, inp, xpos, ypos, stride, contracted=False):
    """``shift_cuda_backward`` (.cu:433-523): (grad_input, grad_xpos, grad_ypos, gxb, gyb), the
    last two the per-element products the reductions consumed."""
    import torch
    H = np.asarray(inp).shape[2]
    gin = bottom_backward(gout, xpos, ypos, H, stride, contracted)
    gxb, gyb = position_backward(inp, gout, xpos, ypos, stride, contracted)

    def reduce(t):                                                 # .cu:501-509
        chw = torch.mean(torch.from_numpy(t), 0, False)
        return torch.sum(torch.sum(chw, 2, False), 1, False).numpy()

    gx, gy = constraint(reduce(gxb), reduce(gyb), contracted)
    return gin, gx, gy, gxb, gyb


class _ShiftCuda:
    """The reference binding's surface (``shift_cuda.forward`` / ``.backward``) on CPU
    tensors, running the compiled reference kernels."""

    def __init__(self, contracted=False):
        self.contracted = contracted

    def forward(self, inp, xpos, ypos, stride):
        import torch
        return torch.from_numpy(forward(inp.detach().numpy(), xpos.detach().numpy(),
                                        ypos.detach().numpy(), stride, self.contracted))

    def backward(self, gout, inp, out, xpos, ypos, stride):
        import torch
        gin, gx, gy, _, _ = backward(gout.detach().numpy(), inp.detach().numpy(),
                                     xpos.detach().numpy(), ypos.detach().numpy(), stride,
                                     self.contracted)
        return [torch.from_numpy(gin), torch.from_numpy(gx), torch.from_numpy(gy)]


def shift_cuda_module(contracted: bool = False):
    _need(contracted)
    return _ShiftCuda(contracted)
