"""Feeder augmentations on the host (shiftgcn.augment) against the reference's own
``feeders.feeder.Feeder`` output (tests/golden/augment_fixtures.npz, written by
tests/golden/gen_augment_fixtures.py): the draws, the numpy path, the AugmentedFeeder and the
CPU form of the DeviceBatchLoader. Every case runs its six clips in order under ONE seed, so
the order of the draws across samples is checked as well."""
import json
import pickle

import numpy as np
import pytest
import torch

from shiftgcn.augment import (MAX_NODES, AugmentedFeeder, AugmentParams, ClipAugment,
                              batch_extents, valid_extent)
from shiftgcn.feeder import DeviceBatchLoader, Feeder

T = 20


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("augment_fixtures.npz")
    return {k: z[k] for k in z.files}


def cases(fx):
    return json.loads(str(fx["cases"]))


CASE_NAMES = ["norm", "shift", "norm_shift", "choose12", "choose20", "choose28", "window12",
              "window28", "shift_choose12", "move1", "move124", "all12", "all20", "all28"]


def make_augment(fx, name):
    choose, shift, move, window, norm, mt, seed = cases(fx)[name]
    kw = {"move_time_candidate": mt} if mt is not None else {}
    return ClipAugment(bool(choose), bool(shift), bool(move), window, bool(norm),
                       fx["mean_map"] if norm else None, fx["std_map"] if norm else None,
                       seed=seed, **kw)


def write_dataset(tmp_path, data):
    dp, lp = tmp_path / "data.npy", tmp_path / "label.pkl"
    np.save(dp, data)
    with open(lp, "wb") as f:
        pickle.dump(([f"clip{i}" for i in range(len(data))], list(range(len(data)))), f)
    return str(dp), str(lp)


def assert_matches(got, want, move):
    """Bit-equal, dtype included. (With random_move the host path restates the reference's
    own np.dot call frame by frame, so equality is asserted there too.)"""
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), \
        f"max |diff| {np.abs(got - want).max()} (move={move})"


def test_fixture_covers_the_named_cases(fx):
    assert sorted(cases(fx)) == sorted(CASE_NAMES)
    d = fx["data"]
    assert d.shape == (6, 3, T, 5, 2) and d.dtype == np.float32
    assert valid_extent(d[0]) == (3, 16) and valid_extent(d[1]) == (0, T)
    assert valid_extent(d[2]) == (0, T) and valid_extent(d[3]) == (5, 18)
    # clip 5 equals the mean map in frames 0-3 and 17-19: the NORMALISED extents differ
    ext = batch_extents(d, fx["mean_map"], fx["std_map"])
    assert ext == [(0, T)] * 5 + [(4, 17)]
    assert batch_extents(d) == [valid_extent(c) for c in d]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_apply_host_matches_reference(fx, name):
    aug = make_augment(fx, name)
    want = fx[f"out_{name}"]
    for i, clip in enumerate(fx["data"]):
        assert_matches(aug.apply_host(clip), want[i], aug.random_move)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_draw_reproduces_recorded_parameters(fx, name):
    aug = make_augment(fx, name)
    data = fx["data"]
    ext = aug.batch_extents(data) if aug.needs_extents else len(data)
    p = aug.draw(ext, T)
    assert isinstance(p, AugmentParams) and len(p) == len(data)
    assert p.T == T and p.T_out == fx[f"out_{name}"].shape[2] == aug.T_out(T)
    assert np.array_equal(p.bias, fx[f"bias_{name}"])
    assert np.array_equal(p.window_begin, fx[f"wbegin_{name}"])
    fm = p.frame_map.astype(np.int64)
    assert (fm >= 0).all() and (fm[:, 1] + fm[:, 2] <= p.T_out).all()
    assert (fm[:, 0] + fm[:, 2] <= T).all()
    if aug.random_move:
        assert np.array_equal(p.move_time, fx[f"mtime_{name}"])
        assert np.array_equal(p.nodes[:, 0], fx[f"nn_{name}"])
        assert p.move.dtype == np.float64 and np.array_equal(p.move, fx[f"move_{name}"])
        for i in range(len(p)):
            nn = p.nodes[i, 0]
            assert p.nodes[i, 1] == 0 and p.nodes[i, nn] == p.T_out
    # the packed buffer is the three tables back to back
    raw = p.pack()
    o_move, o_map, o_nodes = p.offsets()
    assert raw.dtype == np.uint8 and raw.size == AugmentParams.packed_nbytes(len(p))
    assert np.array_equal(raw[o_move:o_map].view(np.float64).reshape(p.move.shape), p.move)
    assert np.array_equal(raw[o_map:o_nodes].view(np.int32).reshape(-1, 3), p.frame_map)
    assert np.array_equal(raw[o_nodes:].view(np.int32).reshape(p.nodes.shape), p.nodes)


@pytest.mark.parametrize("name", ["shift", "shift_choose12", "choose12", "choose28",
                                  "window12", "window28"])
def test_frame_map_is_the_composition_of_shift_and_window(fx, name):
    """The one {src0, dst0, count} map, applied to the clip, is steps 2-3 of the reference."""
    aug = make_augment(fx, name)
    data = fx["data"]
    p = aug.draw(aug.batch_extents(data) if aug.needs_extents else len(data), T)
    for i, clip in enumerate(data):
        src0, dst0, count = p.frame_map[i]
        out = np.zeros((3, p.T_out, 5, 2))
        out[:, dst0:dst0 + count] = clip[:, src0:src0 + count]
        assert np.array_equal(out, fx[f"out_{name}"][i])


@pytest.mark.parametrize("name", ["norm", "all12", "window28", "move124"])
def test_augmented_feeder_getitem_and_maps(fx, tmp_path, name):
    choose, shift, move, window, norm, mt, seed = cases(fx)[name]
    dp, lp = write_dataset(tmp_path, fx["data"])
    kw = {"move_time_candidate": mt} if mt is not None else {}
    fd = AugmentedFeeder(dp, lp, random_choose=bool(choose), random_shift=bool(shift),
                         random_move=bool(move), window_size=window, normalization=bool(norm),
                         seed=seed, **kw)
    assert isinstance(fd, Feeder) and isinstance(fd.augment, ClipAugment)
    if norm:
        for got, want in ((fd.mean_map, fx["mean_map"]), (fd.std_map, fx["std_map"])):
            assert got.dtype == want.dtype and got.shape == (3, 1, 5, 1)
            assert np.array_equal(got, want)
    for i in range(len(fd)):
        x, label, index = fd[i]
        assert label == i and index == i
        assert_matches(x, fx[f"out_{name}"][i], bool(move))


def test_seed_none_takes_the_global_streams(fx):
    import random
    outs = []
    for _ in range(2):
        random.seed(5)
        np.random.seed(5)
        aug = ClipAugment(random_shift=True, random_move=True)
        outs.append(aug.apply_host(fx["data"][0]))
    assert np.array_equal(outs[0], outs[1])


def test_value_errors(fx):
    with pytest.raises(ValueError, match="window_size"):
        ClipAugment(random_choose=True)
    with pytest.raises(ValueError, match="nodes"):
        ClipAugment(random_move=True, move_time_candidate=[1, 9])
    ClipAugment(random_move=True, move_time_candidate=[8])
    with pytest.raises(ValueError, match=r"\(C,1,V,1\)"):
        ClipAugment(normalization=True)
    with pytest.raises(ValueError, match=r"\(C,1,V,1\)"):
        ClipAugment(normalization=True, mean_map=np.zeros((3, 5), np.float32),
                    std_map=np.ones((3, 5), np.float32))
    aug = ClipAugment(normalization=True, mean_map=np.zeros((3, 1, 4, 1), np.float32),
                      std_map=np.ones((3, 1, 4, 1), np.float32))
    with pytest.raises(ValueError, match="maps"):
        aug.apply_host(fx["data"][0])                      # V = 5, maps for V = 4
    with pytest.raises(ValueError, match="C >= 2"):
        ClipAugment(random_move=True).apply_host(np.ones((1, 4, 3, 1), np.float32))
    with pytest.raises(ValueError, match="begin, end"):
        ClipAugment(random_shift=True).draw(3, T)
    with pytest.raises(ValueError, match="extent"):
        ClipAugment(random_shift=True).draw([(5, 5)], T)
    assert MAX_NODES == 9


def test_plain_feeder_still_refuses_and_names_the_replacement(fx, tmp_path):
    dp, lp = write_dataset(tmp_path, fx["data"])
    with pytest.raises(NotImplementedError, match="AugmentedFeeder"):
        Feeder(dp, lp, random_move=True)
    with pytest.raises(NotImplementedError):
        Feeder(dp, lp, window_size=12)


def test_dataloader_collates_augmented_feeder(fx, tmp_path):
    dp, lp = write_dataset(tmp_path, fx["data"])
    fd = AugmentedFeeder(dp, lp, random_choose=True, random_shift=True, random_move=True,
                         window_size=12, normalization=True, seed=22,
                         move_time_candidate=[1, 2, 4])
    dl = torch.utils.data.DataLoader(fd, batch_size=3, shuffle=False, num_workers=0)
    got = list(dl)
    assert len(got) == 2
    x = torch.cat([b[0] for b in got])
    assert x.shape == (6, 3, 12, 5, 2) and x.dtype == torch.float64
    assert np.array_equal(x.numpy(), fx["out_all12"])      # sequential order = fixture order
    assert torch.cat([b[2] for b in got]).tolist() == list(range(6))


@pytest.mark.parametrize("name", ["all12", "norm_shift", "choose28", "move1"])
def test_device_loader_cpu_applies_augment(fx, tmp_path, name):
    """device='cpu': the loader runs the host path with the batch's draws; in loader order
    under one seed that is the sequential reference run, cast to float32 once."""
    choose, shift, move, window, norm, mt, seed = cases(fx)[name]
    dp, lp = write_dataset(tmp_path, fx["data"])
    kw = {"move_time_candidate": mt} if mt is not None else {}
    fd = AugmentedFeeder(dp, lp, random_choose=bool(choose), random_shift=bool(shift),
                         random_move=bool(move), window_size=window, normalization=bool(norm),
                         seed=seed, **kw)
    want = fx[f"out_{name}"].astype(np.float32)
    got = list(DeviceBatchLoader(fd, 4, device="cpu"))     # batches of 4 and 2
    assert [tuple(b[0].shape[:1]) for b in got] == [(4,), (2,)]
    x = torch.cat([b[0] for b in got])
    assert x.dtype == torch.float32 and np.array_equal(x.numpy(), want, equal_nan=True)
    assert torch.cat([b[1] for b in got]).tolist() == list(range(6))
    assert torch.cat([b[2] for b in got]).tolist() == list(range(6))
    # an explicit augment wins over the feeder's, and a plain Feeder takes one too
    plain = Feeder(dp, lp)
    aug = make_augment(fx, name)
    x2 = torch.cat([b[0] for b in DeviceBatchLoader(plain, 6, device="cpu", augment=aug)])
    assert np.array_equal(x2.numpy(), want, equal_nan=True)
    # no augment: today's batches
    x3 = torch.cat([b[0] for b in DeviceBatchLoader(plain, 4, device="cpu")])
    assert np.array_equal(x3.numpy(), fx["data"])


def test_library_binds_clip_augment():
    from test_capi import declared_symbols
    from shiftgcn import _lib
    assert "sgcn_clip_augment" in declared_symbols()
    lib = _lib.load()
    res, args = _lib.SIGNATURES["sgcn_clip_augment"]
    assert len(args) == 16 and lib.sgcn_clip_augment.argtypes == args
    assert lib.sgcn_abi_version() == 25
    # refusals need no device: nothing is enqueued
    nul = [None] * 7
    assert lib.sgcn_clip_augment(*nul, 1, 3, 20, 20, 5, 2, 9, 0, None) == _lib.EINVAL


def test_loader_names_a_stale_library(tmp_path):
    """A library of the same ABI version without the entry (built from an older tree) is a
    NativeLibraryError that says to rebuild, not an AttributeError."""
    import os
    import subprocess
    from conftest import REPO
    from shiftgcn import _lib
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    src = os.path.join(REPO, "shift-gcn_amd", "csrc", "version.hip")
    out = tmp_path / "libshiftgcn_old.so"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared",
                    src, "-o", str(out)], check=True)
    with pytest.raises(_lib.NativeLibraryError, match="rebuild it"):
        _lib._open(str(out))


def test_batch_extents_equal_the_normalised_clip_extents():
    """The compare-only pass plus the boundary check gives the extents of the clip that
    apply_host normalises, also where a quotient underflows to zero (frame 0 below), where a
    whole clip does, and where std == 0 makes x == mean a nan (non-zero)."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((4, 3, 8, 5, 2)).astype(np.float32)
    mean = rng.standard_normal((3, 1, 5, 1)).astype(np.float32)
    mean[0, 0, 0, 0] = mean[1, 0, 2, 0] = 0.5      # one ulp (6e-8) over 3e38 rounds to zero
    std = np.full((3, 1, 5, 1), 3e38, np.float32)
    x[0, :, 0] = np.broadcast_to(mean[:, 0], (3, 5, 2))      # equal to the mean
    x[0, :, 1] = np.broadcast_to(mean[:, 0], (3, 5, 2))
    x[0, 0, 1, 0, 0] = np.nextafter(mean[0, 0, 0, 0], np.float32(9))   # differs by one ulp:
    x[1] = np.broadcast_to(mean, (3, 8, 5, 2))                         # the quotient underflows
    x[1, 1, 3, 2, 1] = np.nextafter(mean[1, 0, 2, 0], np.float32(9))   # ... everywhere
    x[2, :, 6:] = np.broadcast_to(mean, (3, 2, 5, 2))
    std0 = std.copy()
    std0[2, 0, 4, 0] = 0
    for s in (std, std0, np.ones_like(std)):
        with np.errstate(all="ignore"):
            want = [valid_extent((c - mean) / s) for c in x]
        assert batch_extents(x, mean, s) == want
    with np.errstate(all="ignore"):
        assert valid_extent((x[0] - mean) / std)[0] == 2             # frames 0 and 1 are zero
        assert valid_extent((x[1] - mean) / std) == (0, 8)           # all zero after all
        assert valid_extent((x[2] - mean) / std0) == (0, 8)          # nan in every frame
