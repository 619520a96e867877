"""Golden fixtures for the sequence pipeline (window table, skeleton pre-normalisation,
per-frame aggregation, fall intervals), made by running the REFERENCE's own
``create_sliding_windows`` / ``pre_normalize`` / ``run_ensemble_inference`` /
``aggregate_per_frame`` / ``detect_fall_intervals`` (``inference_pipeline.py``) and, for
the NTU joints, ``data_gen/preprocess.pre_normalization`` on CPU. Run only where
``/root/reference`` exists:

    python tests/golden/gen_pipeline_fixtures.py

cv2 and mediapipe (and tqdm when absent) are replaced by stub modules exactly as in
``gen_ensemble_fixtures.py``; the end-to-end case uses that file's formula-weight models.
Only data is stored: the input sequences (not the windows) and the reference's outputs.
The float32-input results of ``pre_normalize`` go to a file of their own, and so do the
float64-input results, stored as their float32-rounded difference from the float32-input
ones (``*_d64``; the sum of the two restores them to ~1e-14), so that each file stays near
half a megabyte.

Every non-empty window must have both rotation angles in [0.2, pi - 0.2] (the arccos of a
float32 cosine is ill-conditioned near alignment, where "no further from float64 than
twice the float32 reference" would say nothing): the seed of a case is searched with the
oracle's angles, and the angles of the chosen sequence are then asserted with the
reference's own ``_angle_between`` / ``_rotation_matrix`` (``angle_between`` /
``rotation_matrix`` for the NTU joints). "Frame sums to zero" must agree with "frame is all
zero" on every frame; that is asserted too.

Output: ``tests/golden/pipeline_fixtures.npz`` (sequences, tables, aggregation, intervals,
the end-to-end case), ``pipeline_fixtures_ref32.npz`` and ``pipeline_fixtures_f64.npz``.
"""
from __future__ import annotations

import contextlib
import io
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import formula  # noqa: E402
import gen_fixtures as gf  # noqa: E402
import pipeline_oracle as po  # noqa: E402

REF = gf.REF
FPS = 30.0
E2E_W, E2E_STRIDE, E2E_T = 64, 32, 200
# with the default weights the formula models' fused scores saturate at 1 - 1e-6 for every
# window; a tenth of them keeps the scores in (0.6, 0.9), where windows differ
E2E_WEIGHTS = (0.06, 0.06, 0.04, 0.04)


def sequence(seed, T, V=33, M=1):
    """A pose (one value per channel and joint, scale 1) plus per-frame motion."""
    pose = formula.tensor((3, 1, V, 1), seed, 1.0).numpy()
    move = formula.tensor((3, T, V, M), seed + 1, 0.25).numpy()
    shift = formula.tensor((3, 1, 1, M), seed + 2, 0.5).numpy()
    return (pose + move + shift).astype(np.float32)


def null(seq, *runs, person=None):
    for a, b in runs:
        if person is None:
            seq[:, a:b] = 0.0
        else:
            seq[:, a:b, :, person] = 0.0
    return seq


def zero_joints(seq):
    seq[:, [0, 3, 4], 7] = 0.0
    seq[:, 30, 11] = 0.0
    seq[:, 41, 23] = 0.0
    return seq


# name -> (W, stride, skeleton, T, V, M, edit)
CASES = {
    "plain": (48, 24, "mp", 131, 33, 1, lambda s: s),
    "nullruns": (48, 24, "mp", 131, 33, 1,
                 lambda s: null(s, (0, 5), (30, 33), (60, 110), (125, 131))),
    "allnull": (48, 24, "mp", 101, 33, 1, lambda s: null(s, (48, 100))),
    "l1": (48, 24, "mp", 80, 33, 1, lambda s: null(s, (25, 72))),
    "short": (48, 24, "mp", 20, 33, 1, lambda s: s),
    "exact96": (48, 24, "mp", 96, 33, 1, lambda s: s),
    "exact72": (48, 24, "mp", 72, 33, 1, lambda s: s),
    "joints": (48, 24, "mp", 60, 33, 1, zero_joints),
    "w70": (70, 35, "mp", 100, 33, 1, lambda s: null(s, (0, 3), (40, 45), (90, 100))),
    "w300": (300, 150, "mp", 300, 33, 1, lambda s: null(s, (100, 104), (270, 300))),
    "ntu_p1absent": (40, 20, "ntu", 40, 25, 2, lambda s: null(s, (0, 40), person=1)),
    "ntu_p1late": (40, 20, "ntu", 40, 25, 2, lambda s: null(s, (0, 12), person=1)),
    "ntu_early": (40, 20, "ntu", 40, 25, 2,
                  lambda s: null(null(s, (29, 40), person=0), (23, 40), person=1)),
    "ntu_empty": (40, 20, "ntu", 40, 25, 2, lambda s: null(s, (0, 40))),
}
SKELETONS = {"mp": po.MEDIAPIPE, "ntu": po.NTU}


def angles_ok(seq, W, stride, skel):
    table = po.sliding_window_table(seq.shape[1], W, stride)
    for raw in po.cut_windows(seq, table, W):
        if not raw.any():
            continue
        if not all(0.2 <= a <= math.pi - 0.2 for a in po.rotation_angles(raw, skel)):
            return False
    return True


def build_sequence(name, seed0):
    W, stride, skel, T, V, M, edit = CASES[name]
    for seed in range(seed0, seed0 + 3000, 3):
        seq = edit(sequence(seed, T, V, M))
        if angles_ok(seq, W, stride, SKELETONS[skel]):
            return seq
    raise AssertionError(f"{name}: no seed gives well-conditioned rotations")


def check_null_frames(wins):
    fr = np.transpose(wins, (0, 4, 2, 3, 1))                    # (N, M, T, V, C)
    assert np.array_equal(fr.sum(-1).sum(-1) == 0, ~fr.any(axis=(-1, -2)))
    assert np.array_equal(np.array([[[f.sum() == 0 for f in p] for p in s] for s in fr]),
                          ~fr.any(axis=(-1, -2)))
    assert np.array_equal(np.array([[p.sum() == 0 for p in s] for s in fr]),
                          ~fr.any(axis=(-1, -2, -3)))


def intervals_arrays(out, key, det):
    out[f"{key}_iv_frames"] = np.array(
        [[d["start_frame"], d["end_frame"], d["peak_frame"]] for d in det],
        dtype=np.int64).reshape(-1, 3)
    out[f"{key}_iv_conf"] = np.array(
        [[d["mean_confidence"], d["peak_confidence"]] for d in det],
        dtype=np.float64).reshape(-1, 2)
    out[f"{key}_iv_times"] = np.array(
        [[d["start_time"], d["end_time"]] for d in det], dtype="U16").reshape(-1, 2)


def main():
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    ref_sg, _ = gf._import_reference()
    stubs = ["cv2", "mediapipe"]
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda x, *a, **k: x
        sys.modules["tqdm"] = t
    for name in stubs:
        sys.modules.setdefault(name, types.ModuleType(name))
    for p in (REF, os.path.join(REF, "data_gen")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import inference_pipeline as ip  # noqa: E402
    import preprocess as ntu_pre  # noqa: E402

    def ref_normalize(wins, skel):
        if skel == "mp":
            return ip.pre_normalize(wins.copy())
        with contextlib.redirect_stdout(io.StringIO()), \
                contextlib.redirect_stderr(io.StringIO()):
            return ntu_pre.pre_normalization(wins.copy())

    def assert_reference_angles(stacked, skel):
        """Both angles of every non-empty window, by the reference's own helpers, from the
        padded and centred frame 0 (the oracle's stages 1 + 2; its whole chain is bit-equal
        to the reference's on every case: tests/test_oracle_pipeline.py)."""
        angle, matrix = ((ip._angle_between, ip._rotation_matrix) if skel == "mp" else
                         (ntu_pre.angle_between, ntu_pre.rotation_matrix))
        joints = SKELETONS[skel]
        for raw in stacked:
            if not raw.any():
                continue
            frame0 = po.normalize_window(raw, joints, 3)[:, 0, :, 0].T        # (V, 3)
            vz = frame0[joints["zaxis"][1]] - frame0[joints["zaxis"][0]]
            az = angle(vz, [0, 0, 1])
            present = frame0.sum(-1) != 0
            turned = frame0.copy()
            turned[present] = np.dot(frame0[present], matrix(np.cross(vz, [0, 0, 1]), az).T)
            ax = angle(turned[joints["xaxis"][0]] - turned[joints["xaxis"][1]], [1, 0, 0])
            assert 0.2 <= az <= math.pi - 0.2 and 0.2 <= ax <= math.pi - 0.2, (az, ax)

    def ref_windows(seq, W, stride):
        wins = ip.create_sliding_windows(seq, window_size=W, stride=stride)
        table = np.array([[s, r] for _, s, _, r in wins], dtype=np.int32)
        assert all(e == s + r for _, s, e, r in wins)
        return wins, table, np.stack([w for w, *_ in wins])

    out32, out64 = {}, {}
    out = {"case_names": np.array(list(CASES), dtype="U16"), "fps": np.float64(FPS)}
    for k, name in enumerate(CASES):
        W, stride, skel, T, V, M, _ = CASES[name]
        seq = build_sequence(name, 4001 + 97 * k)
        wins, table, stacked = ref_windows(seq, W, stride)
        check_null_frames(stacked)
        assert_reference_angles(stacked, skel)
        r32 = ref_normalize(stacked, skel)
        r64 = ref_normalize(stacked.astype(np.float64), skel)
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        scores = 0.5 + formula.hash_uniform(len(wins), 9001 + k)
        per_frame = ip.aggregate_per_frame(
            [(float(sc), s, e, r) for sc, (_, s, e, r) in zip(scores, wins)], T)
        out[f"{name}_seq"] = seq
        out[f"{name}_cfg"] = np.array([W, stride, 0 if skel == "mp" else 1], dtype=np.int32)
        out[f"{name}_table"] = table
        out32[f"{name}_ref32"] = r32
        out64[f"{name}_d64"] = (r64 - r32.astype(np.float64)).astype(np.float32)
        out[f"{name}_scores"] = scores
        out[f"{name}_per_frame"] = per_frame
        intervals_arrays(out, name, ip.detect_fall_intervals(per_frame, 0.5, FPS))
        print(name, table.tolist(), "max|ref32 - ref64| =",
              float(np.abs(r32 - r64).max()))

    # end to end: windows -> pre_normalize -> run_ensemble_inference -> aggregate -> intervals
    graph_mod = types.ModuleType("fixture_graph")

    class Graph:
        def __init__(self, **kw):
            self.A = np.zeros((3, 1, 1))

    graph_mod.Graph = Graph
    sys.modules["fixture_graph"] = graph_mod
    models = {}
    for k, s in enumerate(ip.MODALITIES):
        with gf._cpu_construction():
            m = ref_sg.Model(num_class=2, num_point=33, num_person=1,
                             graph="fixture_graph.Graph")
        formula.fill_state(m, seed=701 + 13 * k)
        models[s] = m.eval()
    CASES["e2e"] = (E2E_W, E2E_STRIDE, "mp", E2E_T, 33, 1,
                    lambda s: null(s, (0, 4), (70, 75), (150, 170)))
    seq = build_sequence("e2e", 7001)
    wins, table, stacked = ref_windows(seq, E2E_W, E2E_STRIDE)
    check_null_frames(stacked)
    assert_reference_angles(stacked, "mp")
    normed = ip.pre_normalize(stacked.copy())
    windows = [(normed[i], s, e, r) for i, (_, s, e, r) in enumerate(wins)]
    cuda0 = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        res = ip.run_ensemble_inference(windows, models, list(E2E_WEIGHTS))
    finally:
        torch.Tensor.cuda = cuda0
    per_frame = ip.aggregate_per_frame(res, E2E_T)
    levels = np.unique(per_frame)
    gaps = np.diff(levels)
    g = int(np.argmax(gaps))
    assert gaps[g] >= 1e-3, gaps
    thr = float(0.5 * (levels[g] + levels[g + 1]))
    out["e2e_seq"] = seq
    out["e2e_cfg"] = np.array([E2E_W, E2E_STRIDE, 0], dtype=np.int32)
    out["e2e_table"] = table
    out["e2e_scores"] = np.array([r[0] for r in res], dtype=np.float64)
    out["e2e_per_frame"] = per_frame
    out["e2e_weights"] = np.array(E2E_WEIGHTS, dtype=np.float64)
    out["e2e_threshold"] = np.float64(thr)
    intervals_arrays(out, "e2e", ip.detect_fall_intervals(per_frame, thr, FPS))
    print("e2e", table.tolist(), out["e2e_scores"], "gap", float(gaps[g]), "thr", thr,
          out["e2e_iv_frames"].tolist())

    for fname, arrays in (("pipeline_fixtures.npz", out), ("pipeline_fixtures_ref32.npz", out32),
                          ("pipeline_fixtures_f64.npz", out64)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
