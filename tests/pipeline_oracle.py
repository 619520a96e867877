"""Numpy restatement of the sequence front end and back end of the inference product:
the window table, the skeleton pre-normalisation of every zero-padded window in closed
form, the per-frame score average and the fall intervals.

Reference: ``inference_pipeline.py:252-281`` (``create_sliding_windows``), ``:167-245``
(``pre_normalize`` = ``data_gen/preprocess.py:8-91`` with the MediaPipe joints),
``:377-386`` (``aggregate_per_frame``) and ``:389-424`` (``detect_fall_intervals``).

The reference pads and normalises with Python loops over window x person x frame. The
closed form here (and in ``csrc/sequence.hip``) is, per window and person:

1. raw[t] = seq[:, start + t] for t < num_real, else 0; a frame is null when all of its
   V*3 values are 0 (the reference tests ``frame.sum() == 0``: the same unless the values
   of a frame cancel);
2. an all-null person stays 0; when raw[0] is null the non-null frames move to the front
   in order;
3. with L the start of the trailing run of null frames, 0 < L < W: frame t >= L is frame
   (t - L) mod L; null frames before L stay 0;
4. (stage 2) p = (p - centre[t]) * ((x + y) + z != 0), centre[t] = person 0's padded
   centre joint (one joint, or (a + b) / 2 of two) at frame t;
5. (stage 4) every joint with (x + y) + z != 0 is rotated, in float64 and rounded back,
   by the Rodrigues matrix that turns person 0's frame-0 bone z_top - z_bottom onto the z
   axis, then by the one that turns x_right - x_left of the rotated frame 0 onto the x axis.

``stages`` is the kernel's bit mask (1 = pad, 2 = centre, 4 = rotate); ``fp64=True`` keeps
every value in float64 (the error-bar reference).
"""
from __future__ import annotations

import math

import numpy as np

MEDIAPIPE = dict(zaxis=(23, 11), xaxis=(12, 11), center=(23, 24))
NTU = dict(zaxis=(0, 1), xaxis=(8, 4), center=(1,))


def sliding_window_table(T, window_size=300, stride=150):
    """int32 (n, 2) rows {start, num_real} of ``create_sliding_windows``."""
    if T <= window_size:
        return np.array([[0, T]], dtype=np.int32)
    rows, start = [], 0
    while start < T:
        end = start + window_size
        rows.append((start, min(end, T) - start))
        start += stride
        if end >= T:
            break
    return np.array(rows, dtype=np.int32)


def cut_windows(seq, table, window_size):
    """The zero-padded windows (n, 3, W, V, M) of a sequence (3, T, V, M)."""
    C, T, V, M = seq.shape
    out = np.zeros((len(table), C, window_size, V, M), dtype=seq.dtype)
    for i, (s, r) in enumerate(table):
        out[i, :, :r] = seq[:, s:s + r]
    return out


def source_map(nonnull):
    """Padded frame t of one person reads raw frame src[t] (-1: stays zero), from the
    (W,) bool flags of its raw frames."""
    W = len(nonnull)
    src = np.full(W, -1, dtype=np.int64)
    idx = np.flatnonzero(nonnull)
    if len(idx) == 0:
        return src
    if not nonnull[0]:
        base, L = idx, len(idx)                     # compacted to the front
    else:
        L = int(idx[-1]) + 1
        base = np.where(nonnull[:L], np.arange(L), -1)
    t = np.arange(W)
    src[:] = base[np.where(t < L, t, (t - L) % L)]
    return src


def rotation_about(axis, angle):
    """Float64 matrix of the rotation by ``angle`` about ``axis``, through the unit
    quaternion (cos(angle/2), -sin(angle/2) * axis / |axis|); the identity for an axis or
    an angle below 1e-6. Sums run left to right, as the reference's do."""
    if np.abs(axis).sum() < 1e-6 or abs(angle) < 1e-6:
        return np.identity(3)
    half = angle / 2.0
    unit = axis / math.sqrt(float(axis @ axis))
    qw = math.cos(half)
    qx, qy, qz = -unit * math.sin(half)
    return np.array([
        [qw * qw + qx * qx - qy * qy - qz * qz, 2 * (qx * qy + qw * qz), 2 * (qx * qz - qw * qy)],
        [2 * (qx * qy - qw * qz), qw * qw + qy * qy - qx * qx - qz * qz, 2 * (qy * qz + qw * qx)],
        [2 * (qx * qz + qw * qy), 2 * (qy * qz - qw * qx), qw * qw + qz * qz - qx * qx - qy * qy],
    ])


def align_angle(v, e):
    """Angle between v (in its own precision up to the unit vector) and unit axis ``e``."""
    if np.abs(v).sum() < 1e-6:
        return 0.0
    u = v / np.sqrt(np.dot(v, v))
    return float(np.arccos(np.clip(np.float64(u[e]), -1.0, 1.0)))


def align_matrix(v, e):
    """The float64 matrix that turns v onto axis ``e`` (2: z, 0: x) about v x e."""
    x, y, z = (np.float64(c) for c in v)
    axis = np.array([y, -x, 0.0]) if e == 2 else np.array([0.0, z, -y])
    return rotation_about(axis, align_angle(v, e))


def _rotate(p, mat):
    """p: (3, W, V, M); joints with (x + y) + z != 0 times ``mat`` in float64."""
    mask = (p[0] + p[1]) + p[2] != 0
    pts = np.moveaxis(p, 0, -1)[mask]                       # (K, 3)
    out = p.copy()
    np.moveaxis(out, 0, -1)[mask] = np.dot(pts.astype(np.float64), mat.T)
    return out


def normalize_window(raw, skeleton=MEDIAPIPE, stages=7):
    """One zero-padded window (3, W, V, M) -> its pre-normalised form, same dtype."""
    C, W, V, M = raw.shape
    p = raw.copy()
    if stages & 1:
        for m in range(M):
            nonnull = (raw[:, :, :, m] != 0).any(axis=(0, 2))
            src = source_map(nonnull)
            gathered = raw[..., m][:, np.maximum(src, 0)]
            p[..., m] = np.where((src >= 0)[None, :, None], gathered, 0)
    if stages & 2:
        cj = skeleton["center"]
        centre = p[:, :, cj[0], 0]
        if len(cj) == 2:
            centre = (centre + p[:, :, cj[1], 0]) / p.dtype.type(2)
        mask = (p[0] + p[1]) + p[2] != 0
        p = (p - centre[:, :, None, None]) * mask[None].astype(p.dtype)
    if stages & 4:
        zb, zt = skeleton["zaxis"]
        xr, xl = skeleton["xaxis"]
        p = _rotate(p, align_matrix(p[:, 0, zt, 0] - p[:, 0, zb, 0], 2))
        p = _rotate(p, align_matrix(p[:, 0, xr, 0] - p[:, 0, xl, 0], 0))
    return p


def rotation_angles(raw, skeleton=MEDIAPIPE):
    """(z angle, x angle) of one window, as ``normalize_window`` finds them."""
    p = normalize_window(raw, skeleton, 3)
    zb, zt = skeleton["zaxis"]
    xr, xl = skeleton["xaxis"]
    vz = p[:, 0, zt, 0] - p[:, 0, zb, 0]
    p = _rotate(p, align_matrix(vz, 2))
    return align_angle(vz, 2), align_angle(p[:, 0, xr, 0] - p[:, 0, xl, 0], 0)


def normalize_windows(seq, table, window_size, skeleton=MEDIAPIPE, stages=7, fp64=False):
    """(3, T, V, M) sequence + window table -> (n, 3, W, V, M)."""
    seq = seq.astype(np.float64 if fp64 else np.float32)
    wins = cut_windows(seq, table, window_size)
    return np.stack([normalize_window(w, skeleton, stages) for w in wins]) if len(wins) \
        else wins


def aggregate_per_frame(scores, table, total_frames):
    """Mean of the scores of the windows whose real frames cover each frame (float64; the
    sums run in table order)."""
    ssum = np.zeros(total_frames, dtype=np.float64)
    cnt = np.zeros(total_frames, dtype=np.float64)
    for sc, (s, r) in zip(scores, table):
        ssum[s:s + r] += sc
        cnt[s:s + r] += 1.0
    return ssum / np.maximum(cnt, 1.0)


def _fmt_time(frame, fps):
    minutes, rest = divmod(frame / fps, 60.0)
    return f"{int(minutes)}:{rest:05.2f}"


def detect_fall_intervals(per_frame, threshold, fps):
    """Maximal runs of frames with score > threshold, as the reference's detection dicts."""
    above = np.concatenate([[False], np.asarray(per_frame) > threshold, [False]])
    edges = np.flatnonzero(above[1:] != above[:-1])
    out = []
    for s, e in zip(edges[::2], edges[1::2]):
        reg = per_frame[s:e]
        out.append({"start_frame": int(s), "end_frame": int(e),
                    "start_time": _fmt_time(int(s), fps), "end_time": _fmt_time(int(e), fps),
                    "mean_confidence": float(np.mean(reg)),
                    "peak_confidence": float(np.max(reg)),
                    "peak_frame": int(s + int(np.argmax(reg)))})
    return out
