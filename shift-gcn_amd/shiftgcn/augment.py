"""The reference feeder's training augmentations (``feeders/feeder.py:74-90``,
``feeders/tools.py:32-117``): normalization, ``random_shift``, ``random_choose`` /
``auto_pading`` to ``window_size`` and ``random_move``.

The reference applies them per sample in ``Dataset.__getitem__``: a Python loop over frames
in float64 inside DataLoader workers. Here the arithmetic of a whole batch is ONE streaming
launch (``sgcn_clip_augment``, csrc/augment.hip) and only the random draws stay on the host:

* :class:`ClipAugment` is the transform specification plus its own ``random.Random(seed)``
  and ``np.random.RandomState(seed)``, the streams ``random.seed(seed)`` /
  ``np.random.seed(seed)`` give the reference. :meth:`ClipAugment.draw` makes the
  reference's draws in the reference's order, sample by sample, and returns them as
  :class:`AugmentParams`; :meth:`ClipAugment.apply_device` is the launch;
  :meth:`ClipAugment.apply_host` is the numpy path for one sample and returns what the
  reference returns, dtype included.
* :class:`AugmentedFeeder` is ``feeders.feeder.Feeder`` with the flags accepted: its
  ``__getitem__`` runs ``apply_host`` (so ``torch.utils.data.DataLoader`` behaves as with the
  reference), and ``DeviceBatchLoader`` picks up its ``.augment`` for the device path.

Why the draws need the clip: ``random.randint(0, n)`` consumes a number of words of the
Mersenne Twister that depends on ``n`` (rejection sampling over ``n.bit_length()`` bits), and
``random_shift``'s range is ``T - (end - begin)``, the valid-frame extent of the (normalised)
clip. Stream parity with the reference therefore needs the extents before the draw; they are
one pass over the staged batch on the host (:func:`batch_extents`).

With ``DataLoader(num_workers > 0)`` every worker process inherits a copy of the same RNG
state (as the reference's workers inherit the same ``random`` state); reseed ``.augment`` in a
``worker_init_fn`` for distinct streams.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import _lib, ops
from .feeder import Feeder

MAX_NODES = 9            # include/shiftgcn.h SGCN_AUG_MAX_NODES
FLAG_NORMALIZE = 1       # SGCN_AUG_NORMALIZE
FLAG_MOVE = 2            # SGCN_AUG_MOVE


def valid_extent(clip):
    """``[begin, end)`` of the frames of a ``(C, T, V, M)`` clip that hold any non-zero
    element (``tools.py:109-111``); an all-zero clip gives ``(0, T)``."""
    valid = (np.asarray(clip) != 0).any(axis=(0, 2, 3))
    return int(valid.argmax()), int(len(valid) - valid[::-1].argmax())


def batch_extents(batch, mean_map=None, std_map=None):
    """:func:`valid_extent` of every sample of a ``(B, C, T, V, M)`` batch, of the normalised
    clips when maps are given, without normalising the batch: ``(x - mean) / std`` is
    non-zero only where ``x != mean`` or ``std == 0`` (inf or nan), so the frames holding such
    an element bound the extent from outside in one compare pass; the two boundary frames are
    then normalised exactly as ``apply_host`` does, and only a sample whose boundary frame
    turns out all zero (a quotient that underflowed) is normalised whole."""
    x = np.asarray(batch)
    B, C, T, V, M = x.shape
    if mean_map is None:
        cand = x != 0
    else:
        # against the map tiled to one clip: long contiguous compare loops (broadcasting the
        # (C,1,V,1) map leaves numpy an inner loop of M elements, ten times slower)
        tiled = np.ascontiguousarray(np.broadcast_to(mean_map, (C, T, V, M))).reshape(-1)
        cand = (x.reshape(B, -1) != tiled).reshape(x.shape)
        if (std_map == 0).any():
            cand |= std_map == 0
    valid = cand.reshape(B, C, T, V * M).any(axis=3).any(axis=1)        # (B, T)
    begin = valid.argmax(axis=1)
    end = T - valid[:, ::-1].argmax(axis=1)
    out = [(int(b), int(e)) for b, e in zip(begin, end)]
    if mean_map is not None:
        mean, std = mean_map[:, 0], std_map[:, 0]                       # (C, V, 1)
        with np.errstate(all="ignore"):
            for i, (b, e) in enumerate(out):
                if not valid[i].any():
                    continue                                            # all zero: (0, T)
                if not ((((x[i, :, b] - mean) / std) != 0).any()
                        and (((x[i, :, e - 1] - mean) / std) != 0).any()):
                    out[i] = valid_extent((x[i] - mean_map) / std_map)
    return out


class AugmentParams:
    """The draws of one batch: ``frame_map (B, 3) int32 {src0, dst0, count}``, ``nodes
    (B, 1 + MAX_NODES) int32 {num_node, node[]}``, ``move (B, 4, MAX_NODES) float64
    {A, S, T_x, T_y}``, and the raw draws ``bias`` / ``window_begin`` (``-1`` where the
    reference drew none) and ``move_time``."""

    def __init__(self, B, T, T_out):
        self.T, self.T_out = int(T), int(T_out)
        self.frame_map = np.zeros((B, 3), dtype=np.int32)
        self.nodes = np.zeros((B, 1 + MAX_NODES), dtype=np.int32)
        self.move = np.zeros((B, 4, MAX_NODES), dtype=np.float64)
        self.bias = np.full(B, -1, dtype=np.int64)
        self.window_begin = np.full(B, -1, dtype=np.int64)
        self.move_time = np.zeros(B, dtype=np.int64)
        self.device_buf = None     # the packed tables on the device (set by the loader)

    def __len__(self):
        return self.frame_map.shape[0]

    @staticmethod
    def packed_nbytes(B):
        return B * (4 * MAX_NODES * 8 + 3 * 4 + (1 + MAX_NODES) * 4)

    def offsets(self):
        """Byte offsets of (move, frame_map, nodes) in the packed buffer (float64 first, so
        every table is naturally aligned)."""
        B = len(self)
        o_map = B * 4 * MAX_NODES * 8
        return 0, o_map, o_map + B * 3 * 4

    def pack(self, out=None):
        """The three tables as one uint8 buffer (into ``out``'s first bytes when given)."""
        n = self.packed_nbytes(len(self))
        if out is None:
            out = np.empty(n, dtype=np.uint8)
        _, o_map, o_nodes = self.offsets()
        out[:o_map] = self.move.reshape(-1).view(np.uint8)
        out[o_map:o_nodes] = self.frame_map.reshape(-1).view(np.uint8)
        out[o_nodes:n] = self.nodes.reshape(-1).view(np.uint8)
        return out[:n]


class ClipAugment:
    """Specification and RNGs of the feeder augmentations (module docstring)."""

    def __init__(self, random_choose=False, random_shift=False, random_move=False,
                 window_size=-1, normalization=False, mean_map=None, std_map=None, seed=None,
                 angle_candidate=(-10., -5., 0., 5., 10.), scale_candidate=(0.9, 1.0, 1.1),
                 transform_candidate=(-0.2, -0.1, 0.0, 0.1, 0.2), move_time_candidate=(1,)):
        self.random_choose = bool(random_choose)
        self.random_shift = bool(random_shift)
        self.random_move = bool(random_move)
        self.window_size = int(window_size)
        self.normalization = bool(normalization)
        if self.random_choose and self.window_size <= 0:
            raise ValueError("random_choose needs window_size > 0")
        self.angle_candidate = [float(v) for v in angle_candidate]
        self.scale_candidate = [float(v) for v in scale_candidate]
        self.transform_candidate = [float(v) for v in transform_candidate]
        self.move_time_candidate = [int(v) for v in move_time_candidate]
        if self.random_move:
            if not self.move_time_candidate or min(self.move_time_candidate) < 1:
                raise ValueError("move_time_candidate must hold positive integers")
            if max(self.move_time_candidate) > MAX_NODES - 1:
                raise ValueError(f"random_move takes at most {MAX_NODES} nodes "
                                 f"(move_time <= {MAX_NODES - 1})")
        self.mean_map = self.std_map = None
        if self.normalization:
            if mean_map is None or std_map is None:
                raise ValueError("normalization needs mean_map and std_map of shape (C,1,V,1)")
            self.mean_map, self.std_map = np.asarray(mean_map), np.asarray(std_map)
            for m in (self.mean_map, self.std_map):
                if m.ndim != 4 or m.shape[1] != 1 or m.shape[3] != 1 \
                        or m.shape != self.mean_map.shape:
                    raise ValueError("normalization needs mean_map and std_map of shape "
                                     f"(C,1,V,1), got {m.shape}")
        self.reseed(seed)
        self._maps_dev = {}

    def reseed(self, seed=None):
        """``random.Random(seed)`` and ``np.random.RandomState(seed)``; ``None`` takes one
        seed for each from the global ``random`` / ``np.random`` streams."""
        if seed is None:
            self.py_rng = random.Random(random.getrandbits(64))
            self.np_rng = np.random.RandomState(int(np.random.randint(0, 2 ** 32,
                                                                      dtype=np.uint64)))
        else:
            self.py_rng = random.Random(seed)
            self.np_rng = np.random.RandomState(seed)

    # ---------------------------------------------------------------- specification
    @property
    def needs_extents(self):
        return self.random_shift

    def T_out(self, T):
        """Frames of the augmented clip of a ``T``-frame input."""
        if self.window_size > 0 and (self.random_choose or T < self.window_size):
            return self.window_size
        return int(T)

    def _check_clip_shape(self, C, V):
        if self.random_move and C < 2:
            raise ValueError("random_move needs at least the x and y channels (C >= 2)")
        if self.normalization and self.mean_map.shape != (C, 1, V, 1):
            raise ValueError(f"normalization maps are {self.mean_map.shape}, the clips need "
                             f"({C}, 1, {V}, 1)")

    # ---------------------------------------------------------------- the draws
    def draw(self, extents, T):
        """The reference's draws for a batch, sample by sample in batch order. ``extents``
        holds each sample's valid-frame extent ``(begin, end)`` (only read under
        ``random_shift``; an int batch size is accepted otherwise)."""
        T = int(T)
        if isinstance(extents, (int, np.integer)):
            if self.random_shift:
                raise ValueError("random_shift needs every sample's (begin, end)")
            extents = [None] * int(extents)
        W, To = self.window_size, self.T_out(T)
        p = AugmentParams(len(extents), T, To)
        for i, ext in enumerate(extents):
            src0, dst0, count = 0, 0, T
            if self.random_shift:                              # tools.py:105-117
                if ext is None:
                    raise ValueError("random_shift needs every sample's (begin, end)")
                begin, end = int(ext[0]), int(ext[1])
                if not 0 <= begin < end <= T:
                    raise ValueError(f"extent {(begin, end)} is not inside [0, {T}]")
                count = end - begin
                bias = self.py_rng.randint(0, T - count)
                p.bias[i] = bias
                src0, dst0 = begin, bias
            if self.random_choose and T < W:                   # auto_pading(random_pad=True)
                wb = self.py_rng.randint(0, W - T)
                p.window_begin[i] = wb
                dst0 += wb
            elif self.random_choose and T > W:                 # crop [wb, wb + W)
                wb = self.py_rng.randint(0, T - W)
                p.window_begin[i] = wb
                lo, hi = max(dst0 - wb, 0), min(dst0 - wb + count, W)
                if hi > lo:
                    src0, dst0, count = src0 + (lo - (dst0 - wb)), lo, hi - lo
                else:                                          # the shifted clip missed the crop
                    src0, dst0, count = 0, 0, 0
            # (window_size > 0 without random_choose pads from frame 0: the map is unchanged)
            assert 0 <= dst0 and dst0 + count <= To and 0 <= src0 and src0 + count <= T
            p.frame_map[i] = (src0, dst0, count)
            if self.random_move:                               # tools.py:64-73
                mt = self.py_rng.choice(self.move_time_candidate)
                node = np.arange(0, To, To * 1.0 / mt).round().astype(int)
                node = np.append(node, To)
                nn = len(node)
                if nn > MAX_NODES:
                    raise ValueError(f"random_move takes at most {MAX_NODES} nodes")
                p.move_time[i] = mt
                p.nodes[i, 0] = nn
                p.nodes[i, 1:1 + nn] = node
                for row, cand in enumerate((self.angle_candidate, self.scale_candidate,
                                            self.transform_candidate,
                                            self.transform_candidate)):
                    p.move[i, row, :nn] = self.np_rng.choice(cand, nn)
        return p

    # ---------------------------------------------------------------- host path
    def _normalize_host(self, x):
        if not self.normalization:
            return x
        with np.errstate(all="ignore"):
            return (x - self.mean_map) / self.std_map

    def _apply_drawn(self, x, p, i):
        """Steps 2-4 of sample ``i`` of ``p`` on the (already normalised) clip ``x``."""
        C, T, V, M = x.shape
        To = p.T_out
        src0, dst0, count = (int(v) for v in p.frame_map[i])
        if self.random_shift or To > T:        # the reference went through np.zeros: float64
            y = np.zeros((C, To, V, M))
            y[:, dst0:dst0 + count] = x[:, src0:src0 + count]
        else:                                  # untouched, or a crop (a view, as tools.py:55)
            y = x[:, src0:src0 + count]
        if not self.random_move:
            return y
        nn = int(p.nodes[i, 0])
        node = p.nodes[i, 1:1 + nn]
        a, s, tx, ty = np.zeros(To), np.zeros(To), np.zeros(To), np.zeros(To)
        A, S, TX, TY = (p.move[i, r, :nn] for r in range(4))
        for k in range(nn - 1):
            lo, hi = int(node[k]), int(node[k + 1])
            a[lo:hi] = np.linspace(A[k], A[k + 1], hi - lo) * np.pi / 180
            s[lo:hi] = np.linspace(S[k], S[k + 1], hi - lo)
            tx[lo:hi] = np.linspace(TX[k], TX[k + 1], hi - lo)
            ty[lo:hi] = np.linspace(TY[k], TY[k + 1], hi - lo)
        theta = np.array([[np.cos(a) * s, -np.sin(a) * s],
                          [np.sin(a) * s, np.cos(a) * s]])
        for f in range(To):                    # the reference's np.dot call, frame by frame
            new_xy = np.dot(theta[:, :, f], y[0:2, f, :, :].reshape(2, -1))
            new_xy[0] += tx[f]
            new_xy[1] += ty[f]
            y[0:2, f, :, :] = new_xy.reshape(2, V, M)
        return y

    def apply_host(self, clip, extents=None):
        """One ``(C, T, V, M)`` sample through the chain in numpy, drawing from this object's
        streams: what ``Feeder.__getitem__`` of the reference returns (float64 after a shift
        or a pad, the input's dtype otherwise)."""
        x = np.array(clip)
        if x.ndim != 4:
            raise ValueError(f"clip must be (C, T, V, M), got {x.shape}")
        C, T, V, M = x.shape
        self._check_clip_shape(C, V)
        x = self._normalize_host(x)
        if self.random_shift and extents is None:
            extents = valid_extent(x)
        return self._apply_drawn(x, self.draw([extents], T), 0)

    def apply_host_batch(self, batch, params, dtype=np.float32):
        """``(B, C, T, V, M)`` raw clips with drawn ``params`` -> ``(B, C, T_out, V, M)``
        (the CPU form of :meth:`apply_device`). ``dtype=np.float64`` keeps the move's float64
        result unrounded (every sample then goes through the chain in float64 after the
        float32 normalization; without ``random_move`` the values are the float32 ones)."""
        batch = np.asarray(batch)
        B, C, T, V, M = batch.shape
        self._check_clip_shape(C, V)
        if len(params) != B or params.T != T:
            raise ValueError("params were drawn for another batch shape")
        out = np.empty((B, C, params.T_out, V, M), dtype=dtype)
        for i in range(B):
            x = self._normalize_host(np.array(batch[i]))
            if np.dtype(dtype) == np.float64:
                x = x.astype(np.float64)
            out[i] = self._apply_drawn(x, params, i)
        return out

    def batch_extents(self, batch):
        """Per-sample extents of a raw ``(B, C, T, V, M)`` batch as ``draw`` needs them."""
        if self.normalization:
            return batch_extents(batch, self.mean_map, self.std_map)
        return batch_extents(batch)

    # ---------------------------------------------------------------- device path
    def _device_maps(self, device):
        maps = self._maps_dev.get(device)
        if maps is None:
            if self.mean_map.dtype != np.float32 or self.std_map.dtype != np.float32:
                raise ValueError("the device path normalises in float32: mean_map and std_map "
                                 "must be float32 (as get_mean_map gives for float32 clips)")
            maps = tuple(torch.from_numpy(np.ascontiguousarray(m.reshape(m.shape[0], -1)))
                         .to(device) for m in (self.mean_map, self.std_map))
            self._maps_dev[device] = maps
        return maps

    def apply_device(self, batch, params, out=None):
        """The launch: raw ``(B, C, T, V, M)`` float32 device clips with the draws ``params``
        -> the augmented ``(B, C, T_out, V, M)`` float32 tensor, enqueued on the device's
        current stream. ``params.device_buf`` (the packed tables, already on the device) is
        used when set; otherwise the tables are uploaded here."""
        ops.check_input(batch, "batch")
        if batch.dim() != 5:
            raise ValueError("batch must be (B, C, T, V, M)")
        B, C, T, V, M = batch.shape
        self._check_clip_shape(C, V)
        if len(params) != B or params.T != T:
            raise ValueError("params were drawn for another batch shape")
        To = params.T_out
        shape = (B, C, To, V, M)
        if out is None:
            out = torch.empty(shape, device=batch.device, dtype=torch.float32)
        else:
            ops.check_input(out, "out")
            if tuple(out.shape) != shape or out.device != batch.device:
                raise ValueError(f"out must be {shape} on the batch's device")
        if B == 0:
            return out
        fm = params.frame_map.astype(np.int64)
        if (fm < 0).any() or (fm[:, 1] + fm[:, 2] > To).any() or (fm[:, 0] + fm[:, 2] > T).any():
            raise ValueError("frame map outside the clip")
        buf = params.device_buf
        if buf is None:
            buf = torch.from_numpy(params.pack()).to(batch.device)
        elif buf.device != batch.device or buf.dtype != torch.uint8 \
                or buf.numel() < params.packed_nbytes(B) or not buf.is_contiguous():
            raise ValueError("params.device_buf must be the packed uint8 tables on the device")
        o_move, o_map, o_nodes = params.offsets()
        base = buf.data_ptr()
        flags = 0
        mean = std = None
        if self.normalization:
            flags |= FLAG_NORMALIZE
            mean, std = self._device_maps(batch.device)
        move = nodes = None
        if self.random_move:
            flags |= FLAG_MOVE
            move, nodes = base + o_move, base + o_nodes
        nbytes = 4 * (batch.numel() + out.numel())
        with ops._timed("clip_augment", 0, nbytes, batch):
            rc = _lib.load().sgcn_clip_augment(
                batch.data_ptr(), out.data_ptr(), base + o_map, nodes, move, ops._ptr(mean),
                ops._ptr(std), B, C, T, To, V, M, MAX_NODES, flags, ops._stream(batch))
        _lib.check(rc, "sgcn_clip_augment")
        return out


class AugmentedFeeder(Feeder):
    """``feeders/feeder.py:11-95`` with its augmentation flags accepted. ``__getitem__``
    applies them on the host as the reference does; ``DeviceBatchLoader`` applies the same
    specification (``.augment``) on the device instead. ``seed`` and the ``*_candidate``
    lists are passed to :class:`ClipAugment`."""

    def __init__(self, data_path, label_path, random_choose=False, random_shift=False,
                 random_move=False, window_size=-1, normalization=False, debug=False,
                 use_mmap=True, seed=None, **candidates):
        super().__init__(data_path, label_path, debug=debug, use_mmap=use_mmap)
        self.random_choose = random_choose
        self.random_shift = random_shift
        self.random_move = random_move
        self.window_size = window_size
        self.normalization = normalization
        self.mean_map = self.std_map = None
        if normalization:
            self.get_mean_map()
        self.augment = ClipAugment(random_choose, random_shift, random_move, window_size,
                                   normalization, self.mean_map, self.std_map, seed=seed,
                                   **candidates)

    def get_mean_map(self):
        """``feeder.py:62-66``, the same numpy expressions."""
        data = self.data
        N, C, T, V, M = data.shape
        self.mean_map = np.asarray(
            data.mean(axis=2, keepdims=True).mean(axis=4, keepdims=True).mean(axis=0))
        self.std_map = np.asarray(
            data.transpose((0, 2, 4, 1, 3)).reshape((N * T * M, C * V)).std(axis=0)
            .reshape((C, 1, V, 1)))

    def __getitem__(self, index):
        return self.augment.apply_host(self.data[index]), self.label[index], index
