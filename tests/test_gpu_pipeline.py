"""GPU parity of the sequence pipeline (``shiftgcn.pipeline`` over ``csrc/sequence.hip``)
with the reference's ``create_sliding_windows`` -> ``pre_normalize`` ->
``run_ensemble_inference`` -> ``aggregate_per_frame`` -> ``detect_fall_intervals`` chain
(tests/golden/pipeline_fixtures*.npz) and with the numpy closed form
(tests/pipeline_oracle.py, itself bit-equal to the reference on every fixture case).

Padding and centring are exact; the rotation is held to the project's error-bar form: no
further from the float64 reference than twice the float32 reference is. The float32
reference's own distance is 1.6e-7 ... 4.6e-7 on these cases (coordinates of order 1); the
kernel has the same float32 roundings and may differ by an ulp of |v| and by the device's
acos / sin / cos."""
import numpy as np
import pytest
import torch

import formula
import pipeline_oracle as po
from test_oracle_pipeline import case, case_names, fixture_intervals

pytestmark = pytest.mark.gpu
DEV = "cuda"
SKEL_NAMES = ("MEDIAPIPE", "NTU")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pipeline_fixtures.npz")


@pytest.fixture(scope="module")
def ref32(golden):
    return golden("pipeline_fixtures_ref32.npz")


@pytest.fixture(scope="module")
def f64(golden):
    return golden("pipeline_fixtures_f64.npz")


def _skeleton(fx, name):
    from shiftgcn import pipeline
    return getattr(pipeline, SKEL_NAMES[int(fx[f"{name}_cfg"][2])])


def _normalize(fx, name, stages):
    from shiftgcn import pipeline
    seq, table, W, stride, _ = case(fx, name)
    out = pipeline.normalize_windows(torch.from_numpy(seq).to(DEV), table, W,
                                     _skeleton(fx, name), stages=stages)
    assert out.shape == (len(table), 3, W) + seq.shape[2:] and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("stages", [1, 3])
def test_pad_and_centre_bit_exact(fx, stages):
    for name in case_names(fx):
        seq, table, W, stride, skel = case(fx, name)
        want = po.normalize_windows(seq, table, W, skel, stages=stages)
        assert np.array_equal(_normalize(fx, name, stages), want), name


@pytest.fixture(scope="module")
def normalized(fx):
    return {name: _normalize(fx, name, 7) for name in case_names(fx)}


def test_normalize_zero_pattern(ref32, normalized):
    for name, got in normalized.items():
        assert np.array_equal(got == 0, ref32[f"{name}_ref32"] == 0), name


def test_normalize_within_twice_the_fp32_reference_error(ref32, f64, normalized):
    for name, got in normalized.items():
        d64 = f64[f"{name}_d64"].astype(np.float64)              # ref64 - ref32
        ref64 = ref32[f"{name}_ref32"].astype(np.float64) + d64
        ref_err = float(np.abs(d64).max())
        err = float(np.abs(got.astype(np.float64) - ref64).max())
        print(f"{name}: max|ours - ref64| = {err:.3e}, max|ref32 - ref64| = {ref_err:.3e}")
        assert err <= 2 * ref_err, (name, err, ref_err)


def test_device_table_rows_are_clamped(fx):
    """A table that is already on the device cannot be checked by the host: a row longer
    than the window or past the end of the sequence is cut to what exists."""
    from shiftgcn import pipeline
    seq, _, W, stride, skel = case(fx, "plain")
    T = seq.shape[1]
    bad = torch.tensor([[0, W + 5], [T - 10, W], [T + 3, 4]], dtype=torch.int32, device=DEV)
    good = np.array([[0, W], [T - 10, 10], [T, 0]], dtype=np.int32)
    d_seq = torch.from_numpy(seq).to(DEV)
    got = pipeline.normalize_windows(d_seq, bad, W)
    want = pipeline.normalize_windows(d_seq, good, W)
    assert torch.equal(got, want) and not bool(got[2].any())
    with pytest.raises(ValueError):
        pipeline.normalize_windows(d_seq, bad.cpu().numpy(), W)


def test_empty_table(fx):
    from shiftgcn import pipeline
    seq = torch.from_numpy(fx["short_seq"]).to(DEV)
    out = pipeline.normalize_windows(seq, np.zeros((0, 2), dtype=np.int32), 48)
    assert out.shape == (0, 3, 48, 33, 1)
    per_frame = pipeline.aggregate_per_frame(
        torch.zeros(0, dtype=torch.float64, device=DEV), np.zeros((0, 2), dtype=np.int32), 9)
    assert per_frame.dtype == torch.float64 and per_frame.cpu().tolist() == [0.0] * 9


def test_aggregate_bit_exact(fx):
    from shiftgcn import pipeline
    for name in case_names(fx) + ["e2e"]:
        T = fx[f"{name}_seq"].shape[1]
        got = pipeline.aggregate_per_frame(torch.from_numpy(fx[f"{name}_scores"]).to(DEV),
                                           fx[f"{name}_table"], T)
        assert got.dtype == torch.float64
        assert np.array_equal(got.cpu().numpy(), fx[f"{name}_per_frame"]), name


@pytest.fixture(scope="module")
def ensemble(fx):
    """The formula-weight models of the fixture generator (seeds 701 + 13k)."""
    import shiftgcn
    from shiftgcn import ensemble as ens
    models = []
    for k in range(4):
        m = shiftgcn.Model(num_class=2, num_point=33, num_person=1,
                           graph="graph.mediapipe_pose.Graph")
        formula.fill_state(m, seed=701 + 13 * k)
        models.append(m.to(DEV).eval())
    return ens.Ensemble(models, weights=tuple(fx["e2e_weights"])).to(DEV)


def test_sequence_scorer_matches_reference_chain(fx, ensemble):
    from shiftgcn import pipeline
    seq = fx["e2e_seq"]
    W, stride, _ = (int(v) for v in fx["e2e_cfg"])
    n = len(fx["e2e_table"])
    batch = 4
    assert n % batch                                           # the last chunk is padded
    graphed = pipeline.SequenceScorer(ensemble, W, stride, batch=batch, graph=True)
    eager = pipeline.SequenceScorer(ensemble, W, stride, batch=batch, graph=False)
    per_frame, scores, table = graphed.score(seq)                          # numpy in
    per_frame_e, scores_e, _ = eager.score(torch.from_numpy(seq).to(DEV))  # device tensor in
    assert np.array_equal(table, fx["e2e_table"])
    assert scores.shape == (n,) and per_frame.shape == (seq.shape[1],)
    assert scores.dtype == per_frame.dtype == torch.float64 and per_frame.is_cuda
    assert torch.equal(scores, scores_e) and torch.equal(per_frame, per_frame_e)
    assert np.abs(scores.cpu().numpy() - fx["e2e_scores"]).max() < 1e-5
    assert np.abs(per_frame.cpu().numpy() - fx["e2e_per_frame"]).max() < 1e-5
    # a second sequence replays the same graph
    again = graphed.score(seq)[1]
    assert torch.equal(again, scores) and graphed._graph.captures == 1
    # a sequence with fewer windows than the batch is padded to it: still the same graph
    held = graphed._graph
    short = graphed.score(seq[:, :W + 5])[1]
    assert graphed._graph is held and held.captures == 1
    assert short.shape == (2,) and torch.equal(short, eager.score(seq[:, :W + 5])[1])
    # the threshold sits in the widest gap of the reference's per-frame scores (>= 1e-3 wide)
    got = pipeline.detect_fall_intervals(per_frame, float(fx["e2e_threshold"]), float(fx["fps"]))
    want = fixture_intervals(fx, "e2e")
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        for key in ("start_frame", "end_frame", "start_time", "end_time", "peak_frame"):
            assert g[key] == w[key], key
        for key in ("mean_confidence", "peak_confidence"):
            assert abs(g[key] - w[key]) < 1e-5, key
