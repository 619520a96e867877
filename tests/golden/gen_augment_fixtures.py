"""Fixtures of the feeder augmentations (tests/test_augment_host.py, tests/test_gpu_augment.py).

Run only where a checkout of the reference exists:

    python tests/golden/gen_augment_fixtures.py <path to the reference>

What runs: the reference's own ``feeders.feeder.Feeder`` (and through it ``feeders.tools``)
on a small deterministic clip file, after ``random.seed(seed)`` / ``np.random.seed(seed)``,
item 0, 1, 2, ... in order under ONE seed per case (so every case also checks the order of
the draws across samples). ``random.randint``, ``random.choice`` and ``np.random.choice`` are
wrapped while it runs to record what was drawn. Only the inputs, the seeds, the recorded
draws and the outputs are stored (``augment_fixtures.npz``); nothing of the reference's text.

The clips, ``(C=3, T=20, V=5, M=2)`` float32, values on a 1/256 grid:
  0  leading (3) and trailing (4) zero frames       3  leading, interior and trailing zeros
  1  all zero                                       4  no zero frame
  2  interior zero frames (7-9)                     5  equal to the mean map in frames 0-3, 17-19
Clip 5 is made a fixed point of ``get_mean_map`` (its frames are set to the mean of the file
that contains them), so under normalization its extent is [4, 17) while the zero frames of the
other clips, normalised, are non-zero.
"""
import functools
import json
import os
import pickle
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "augment_fixtures.npz")
C, T, V, M = 3, 20, 5, 2

# name: (random_choose, random_shift, random_move, window_size, normalization, move_time, seed)
CASES = {
    "norm": (0, 0, 0, -1, 1, None, 11),
    "shift": (0, 1, 0, -1, 0, None, 12),
    "norm_shift": (0, 1, 0, -1, 1, None, 13),
    "choose12": (1, 0, 0, 12, 0, None, 14),
    "choose20": (1, 0, 0, 20, 0, None, 15),
    "choose28": (1, 0, 0, 28, 0, None, 16),
    "window12": (0, 0, 0, 12, 0, None, 17),
    "window28": (0, 0, 0, 28, 0, None, 18),
    "shift_choose12": (1, 1, 0, 12, 0, None, 19),
    "move1": (0, 0, 1, -1, 0, [1], 20),
    "move124": (0, 0, 1, -1, 0, [1, 2, 4], 21),
    "all12": (1, 1, 1, 12, 1, [1, 2, 4], 22),
    "all20": (1, 1, 1, 20, 1, [1], 23),
    "all28": (1, 1, 1, 28, 1, [1, 2, 4], 24),
}


def make_clips():
    rng = np.random.default_rng(2024)
    x = (rng.integers(-512, 513, (6, C, T, V, M)) / 256.0).astype(np.float32)
    x[x == 0] = 1 / 256.0                      # zeros only where placed below
    x[0, :, :3] = 0
    x[0, :, 16:] = 0
    x[1] = 0
    x[2, :, 7:10] = 0
    x[3, :, :5] = 0
    x[3, :, 9:11] = 0
    x[3, :, 18:] = 0
    special = list(range(0, 4)) + list(range(17, 20))
    for _ in range(64):                        # clip 5's special frames := the file's mean map
        mean = x.mean(axis=2, keepdims=True).mean(axis=4, keepdims=True).mean(axis=0)
        new = np.broadcast_to(mean, (C, T, V, M))[:, special]
        if np.array_equal(new, x[5][:, special]):
            break
        x[5][:, special] = new
    else:
        raise SystemExit("clip 5 did not reach a fixed point of the mean map")
    return x


def main(ref):
    sys.path.insert(0, ref)
    from feeders import feeder as ref_feeder, tools

    data = make_clips()
    tmp = tempfile.mkdtemp()
    dp, lp = os.path.join(tmp, "data.npy"), os.path.join(tmp, "label.pkl")
    np.save(dp, data)
    with open(lp, "wb") as f:
        pickle.dump(([f"clip{i}" for i in range(len(data))], list(range(len(data)))), f)

    log = []
    orig = (random.randint, random.choice, np.random.choice, tools.random_move)

    def wrap(kind, fn):
        def inner(*a, **k):
            v = fn(*a, **k)
            log.append((kind, v))
            return v
        return inner

    random.randint = wrap("randint", orig[0])
    random.choice = wrap("choice", orig[1])
    np.random.choice = wrap("npchoice", orig[2])

    store = {"data": data, "cases": np.array(json.dumps(CASES))}
    for name, (choose, shift, move, window, norm, mt, seed) in CASES.items():
        tools.random_move = (functools.partial(orig[3], move_time_candidate=mt)
                             if mt is not None else orig[3])
        fd = ref_feeder.Feeder(dp, lp, random_choose=bool(choose), random_shift=bool(shift),
                               random_move=bool(move), window_size=window,
                               normalization=bool(norm))
        if norm:
            store["mean_map"], store["std_map"] = np.asarray(fd.mean_map), np.asarray(fd.std_map)
            z = (data[5] - fd.mean_map) / fd.std_map
            assert not z[:, :4].any() and not z[:, 17:].any() and z[:, 4:17].any(axis=(0, 2, 3)).all()
        random.seed(seed)
        np.random.seed(seed)
        outs = []
        n = len(data)
        bias, wbegin = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        mtime, nn = np.zeros(n, np.int64), np.zeros(n, np.int64)
        mv = np.zeros((n, 4, 9))
        for i in range(n):
            del log[:]
            x, label, index = fd[i]
            assert label == i and index == i
            outs.append(np.array(x))
            ints = [v for k, v in log if k == "randint"]
            if shift:
                bias[i] = ints.pop(0)
            if choose and window != T:
                wbegin[i] = ints.pop(0)
            assert not ints
            if move:
                (mtime[i],) = [v for k, v in log if k == "choice"]
                rows = [v for k, v in log if k == "npchoice"]
                assert len(rows) == 4
                nn[i] = len(rows[0])
                for r, v in enumerate(rows):
                    mv[i, r, :len(v)] = v
        out = np.stack(outs)
        assert out.dtype == outs[0].dtype
        store[f"out_{name}"] = out
        store[f"bias_{name}"], store[f"wbegin_{name}"] = bias, wbegin
        if move:
            store[f"mtime_{name}"], store[f"nn_{name}"], store[f"move_{name}"] = mtime, nn, mv
    random.randint, random.choice, np.random.choice, tools.random_move = orig
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
