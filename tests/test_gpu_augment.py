"""Feeder augmentations on the device: ``sgcn_clip_augment`` (csrc/augment.hip) against the
numpy path of shiftgcn.augment with the SAME drawn parameters, and the DeviceBatchLoader that
launches it on its copy stream against a sequential host run under one seed.

Bars (per element):
* without random_move: bit-equal to ``apply_host(...).astype(float32)`` (IEEE float32
  subtract/divide, a copy through the frame map, exact zeros elsewhere);
* with random_move, channels 0/1: ``|dev - ref| <= 2^-23 |ref| + 2^-48 (1.1 (|x| + |y|) + 0.2)``
  with ``ref`` the float64 host result and ``x, y`` the pre-move operands: one float32
  rounding that may tip across a tie, plus float64 evaluation differences (libm vs device
  sin/cos, FMA) for matrix entries ``<= 1.1`` and translations ``<= 0.2`` (the default
  candidates). A float32 evaluation of the transform misses this under cancellation.
  Channels >= 2 stay bit-equal.
"""
import json
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASE_NAMES = ["norm", "shift", "norm_shift", "choose12", "choose20", "choose28", "window12",
              "window28", "shift_choose12", "move1", "move124", "all12", "all20", "all28"]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("augment_fixtures.npz")
    return {k: z[k] for k in z.files}


def premove(aug, raw, p):
    """Steps 1-3 restated independently of apply_host: float32 normalization, then the frame
    map into zeros. Float64 holding float32 values: the operands of the move."""
    B, C, T, V, M = raw.shape
    pre = np.zeros((B, C, p.T_out, V, M))
    for i in range(B):
        x = raw[i]
        if aug.normalization:
            x = (x - aug.mean_map) / aug.std_map
            assert x.dtype == np.float32
        s, d, c = (int(v) for v in p.frame_map[i])
        pre[i][:, d:d + c] = x[:, s:s + c]
    return pre


def check(dev, ref, pre, move, what=""):
    assert dev.dtype == np.float32 and dev.shape == ref.shape == pre.shape
    if not move:
        assert np.array_equal(dev, ref.astype(np.float32)), what
        assert np.array_equal(dev, pre.astype(np.float32)), what
        return
    assert ref.dtype == np.float64
    assert np.array_equal(dev[:, 2:], pre[:, 2:].astype(np.float32)), what
    mag = 1.1 * (np.abs(pre[:, 0:1]) + np.abs(pre[:, 1:2])) + 0.2
    tol = 2.0 ** -23 * np.abs(ref[:, :2]) + 2.0 ** -48 * mag
    err = np.abs(dev[:, :2].astype(np.float64) - ref[:, :2])
    print(f"{what}: max err/tol {float((err / tol).max()):.3f}, max err {float(err.max()):.3e}")
    assert (err <= tol).all(), what


def poisoned(arr, fill, pad=301):
    """``arr`` on the device inside a larger allocation filled with ``fill``."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    flat = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device="cuda")
    view = flat[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return flat, view


def run_kernel(aug, raw, p):
    """One sgcn_clip_augment launch with every input in a poisoned allocation and the output
    between sentinel margins; returns the output (numpy) after checking the margins."""
    from shiftgcn import _lib
    from shiftgcn.augment import MAX_NODES
    B, C, T, V, M = raw.shape
    nan = float("nan")
    keep = [poisoned(raw, nan), poisoned(p.frame_map, 2 ** 30), poisoned(p.nodes, 2 ** 30),
            poisoned(p.move, nan)]
    x, fm, nodes, move = (v for _, v in keep)
    flags, mean, std = 0, None, None
    if aug.normalization:
        flags |= 1
        keep += [poisoned(aug.mean_map.reshape(C, V), nan),
                 poisoned(aug.std_map.reshape(C, V), nan)]
        mean, std = keep[-2][1], keep[-1][1]
    if aug.random_move:
        flags |= 2
    n_out, pad = B * C * p.T_out * V * M, 4099
    flat = torch.full((n_out + 2 * pad,), SENTINEL, dtype=torch.float32, device="cuda")
    out = flat[pad:pad + n_out].view(B, C, p.T_out, V, M)
    rc = _lib.load().sgcn_clip_augment(
        x.data_ptr(), out.data_ptr(), fm.data_ptr(),
        nodes.data_ptr() if aug.random_move else None,
        move.data_ptr() if aug.random_move else None,
        mean.data_ptr() if mean is not None else None,
        std.data_ptr() if std is not None else None,
        B, C, T, p.T_out, V, M, MAX_NODES, flags, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:pad] == SENTINEL).all() and (host[pad + n_out:] == SENTINEL).all()
    return host[pad:pad + n_out].reshape(B, C, p.T_out, V, M)


def make_augment(fx, name):
    from shiftgcn.augment import ClipAugment
    choose, shift, move, window, norm, mt, seed = json.loads(str(fx["cases"]))[name]
    kw = {"move_time_candidate": mt} if mt is not None else {}
    return ClipAugment(bool(choose), bool(shift), bool(move), window, bool(norm),
                       fx["mean_map"] if norm else None, fx["std_map"] if norm else None,
                       seed=seed, **kw)


def drawn(aug, raw):
    ext = aug.batch_extents(raw) if aug.needs_extents else len(raw)
    return aug.draw(ext, raw.shape[2])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_matches_host_on_fixture_shapes(fx, name):
    """B = 5 of the fixture clips (zeros in front, behind and inside, an all-zero clip, the
    clip equal to the mean map), every fixture configuration."""
    aug = make_augment(fx, name)
    raw = fx["data"][[0, 1, 2, 3, 5]]
    p = drawn(aug, raw)
    dev = run_kernel(aug, raw, p)
    ref = aug.apply_host_batch(raw, p, dtype=np.float64)
    check(dev, ref, premove(aug, raw, p), aug.random_move, name)
    # the public launch gives the same bits
    got = aug.apply_device(torch.from_numpy(raw).cuda(), p)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), dev)


def big_clips(B, T, V, M, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((B, 3, T, V, M)).astype(np.float32)
    raw[0, :, :T // 7] = 0                  # leading zeros
    raw[0, :, T - T // 5:] = 0              # trailing zeros
    if B > 1:
        raw[1, :, T // 2:T // 2 + 3] = 0    # interior zeros only
    mean = rng.uniform(-0.5, 0.5, (3, 1, V, 1)).astype(np.float32)
    std = rng.uniform(0.5, 2.0, (3, 1, V, 1)).astype(np.float32)
    return raw, mean, std


@pytest.mark.parametrize("shape,window,flags", [
    ((2, 300, 25, 2), 64, "csmn"), ((2, 300, 25, 2), 320, "csmn"),
    ((2, 300, 25, 2), 64, "csn"), ((3, 40, 33, 1), -1, "smn"), ((3, 40, 33, 1), 24, "cs"),
])
def test_kernel_matches_host_at_larger_shapes(shape, window, flags):
    """NTU clips (T = 300) cropped to 64 and padded to 320 frames (whole 16-frame tiles,
    several workgroups per sample), and a 33-joint single-person clip (V*M odd) at 40 and 24
    frames (a partial last tile)."""
    from shiftgcn.augment import ClipAugment
    B, T, V, M = shape
    raw, mean, std = big_clips(B, T, V, M, T + V)
    norm = "n" in flags
    aug = ClipAugment("c" in flags, "s" in flags, "m" in flags, window, norm,
                      mean if norm else None, std if norm else None, seed=T + window,
                      move_time_candidate=[1, 2, 4])
    if norm:                                # extents of the NORMALISED clip: equal to the mean
        raw[0, :, :T // 7] = np.broadcast_to(mean, (3, T // 7, V, M))
    p = drawn(aug, raw)
    assert p.T_out == (window if window > 0 else T)
    dev = run_kernel(aug, raw, p)
    ref = aug.apply_host_batch(raw, p, dtype=np.float64)
    check(dev, ref, premove(aug, raw, p), aug.random_move, f"{shape} w{window} {flags}")


def _write(tmp_path, n, T=40, V=25, M=2):
    rng = np.random.default_rng(n)
    data = rng.standard_normal((n, 3, T, V, M)).astype(np.float32)
    for i in range(n):                      # zero frames in front and behind, varying
        data[i, :, :i % 7] = 0
        if i % 5:
            data[i, :, T - i % 5:] = 0
    data[3] = 0
    labels = [int(v) for v in rng.integers(0, 60, n)]
    np.save(tmp_path / "d.npy", data)
    with open(tmp_path / "l.pkl", "wb") as f:
        pickle.dump(([f"s{i}" for i in range(n)], labels), f)
    return str(tmp_path / "d.npy"), str(tmp_path / "l.pkl"), data, labels


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("move", [False, True])
def test_device_loader_equals_sequential_host_run(tmp_path, depth, move):
    from shiftgcn.augment import AugmentedFeeder, ClipAugment
    from shiftgcn.feeder import DeviceBatchLoader, loader_order
    dp, lp, data, labels = _write(tmp_path, 23)
    spec = dict(random_choose=True, random_shift=True, random_move=move, window_size=32,
                normalization=True)
    fd = AugmentedFeeder(dp, lp, seed=77, move_time_candidate=[1, 2, 4], **spec)
    seq = ClipAugment(mean_map=fd.mean_map, std_map=fd.std_map, seed=77,
                      move_time_candidate=[1, 2, 4], **spec)      # sequential apply_host
    bat = ClipAugment(mean_map=fd.mean_map, std_map=fd.std_map, seed=77,
                      move_time_candidate=[1, 2, 4], **spec)      # the operands of the bar
    torch.manual_seed(3)
    want = loader_order(23, 4, True, True)
    torch.manual_seed(3)
    got = []
    for x, y, idx in DeviceBatchLoader(fd, 4, shuffle=True, drop_last=True, device="cuda",
                                       depth=depth):
        assert x.is_cuda and x.dtype == torch.float32 and x.shape == (4, 3, 32, 25, 2)
        assert x.shape[2] == fd.augment.T_out(40)
        x2 = x * 2.0                      # a consumer kernel on the current stream
        torch.cuda.synchronize()
        i = idx.tolist()
        ref = np.stack([seq.apply_host(data[k]) for k in i])
        assert ref.dtype == np.float64
        p = bat.draw(bat.batch_extents(data[i]), 40)
        dev = x.cpu().numpy()
        check(dev, ref, premove(bat, data[i], p), move, f"batch {len(got)}")
        assert np.array_equal(x2.cpu().numpy(), dev * np.float32(2.0))
        assert y.cpu().tolist() == [labels[k] for k in i]
        got.append(i)
    assert got == want and len(got) == 5


def test_loader_without_augment_is_unchanged(tmp_path):
    from shiftgcn.feeder import DeviceBatchLoader, Feeder
    dp, lp, data, labels = _write(tmp_path, 11)
    f = Feeder(dp, lp)
    loader = DeviceBatchLoader(f, 4, shuffle=True, device="cuda", augment=None)
    assert loader.augment is None
    torch.manual_seed(5)
    for x, y, idx in loader:
        torch.cuda.synchronize()
        i = idx.tolist()
        assert x.shape[1:] == (3, 40, 25, 2)
        assert np.array_equal(x.cpu().numpy(), data[i])
        assert y.cpu().tolist() == [labels[k] for k in i]


def test_augmented_batch_feeds_training_step(tmp_path):
    import shiftgcn
    from shiftgcn import train
    from shiftgcn.augment import AugmentedFeeder
    from shiftgcn.feeder import DeviceBatchLoader
    dp, lp, data, labels = _write(tmp_path, 6)
    fd = AugmentedFeeder(dp, lp, random_choose=True, random_shift=True, random_move=True,
                         window_size=16, normalization=True, seed=1)
    torch.manual_seed(1)
    model = shiftgcn.Model(num_class=60, num_point=25, num_person=2,
                           graph="graph.ntu_rgb_d.Graph").cuda().train()
    opt = train.build_optimizer(model, base_lr=0.1)
    it = iter(DeviceBatchLoader(fd, 2, shuffle=True, drop_last=True))
    x, y, _ = next(it)
    assert x.shape == (2, 3, 16, 25, 2)
    loss = float(train.train_step(model, opt, x, y).detach())
    it.close()
    torch.cuda.synchronize()
    assert np.isfinite(loss)


def test_refusals():
    from shiftgcn import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    q = buf.data_ptr()
    o = q + 8192
    dims = (2, 3, 8, 8, 5, 2, 9)            # B, C, T, T_out, V, M, max_nodes
    call = lib.sgcn_clip_augment
    assert call(q, o, q, q, q, q, q, *dims, 3, None) == 0
    torch.cuda.synchronize()
    assert call(None, o, q, q, q, q, q, *dims, 3, None) == _lib.EINVAL
    assert call(q, None, q, q, q, q, q, *dims, 3, None) == _lib.EINVAL
    assert call(q, o, None, q, q, q, q, *dims, 3, None) == _lib.EINVAL
    assert call(q, q, q, q, q, q, q, *dims, 3, None) == _lib.EINVAL      # in-place
    assert call(q, o, q, None, q, q, q, *dims, 2, None) == _lib.EINVAL   # move needs nodes
    assert call(q, o, q, q, None, q, q, *dims, 2, None) == _lib.EINVAL
    assert call(q, o, q, q, q, None, q, *dims, 1, None) == _lib.EINVAL   # normalise needs maps
    assert call(q, o, q, q, q, q, None, *dims, 1, None) == _lib.EINVAL
    assert call(q, o, q, None, None, None, None, *dims, 0, None) == 0    # optional without bits
    assert call(q, o, q, q, q, q, q, *dims, 4, None) == _lib.EINVAL      # unknown flag
    for k in range(6):                                                   # a dimension < 1
        bad = list(dims)
        bad[k] = 0
        assert call(q, o, q, q, q, q, q, *bad, 3, None) == _lib.EINVAL
    assert call(q, o, q, q, q, q, q, 2, 1, 8, 8, 5, 2, 9, 2, None) == _lib.EINVAL   # C < 2
    assert call(q, o, q, q, q, q, q, 2, 3, 8, 8, 5, 2, 10, 2, None) == _lib.EINVAL  # nodes > 9
    assert call(q, o, q, q, q, q, q, 2, 3, 8, 8, 5, 2, 1, 2, None) == _lib.EINVAL
    torch.cuda.synchronize()
