"""The sequence-pipeline oracle (tests/pipeline_oracle.py) against the reference's own
``create_sliding_windows`` / ``pre_normalize`` (``pre_normalization`` for the NTU joints) /
``aggregate_per_frame`` / ``detect_fall_intervals`` outputs (tests/golden/
pipeline_fixtures*.npz, made by gen_pipeline_fixtures.py), and the product's host-side
helpers in ``shiftgcn.pipeline`` against the same fixtures. No GPU."""
import numpy as np
import pytest

import pipeline_oracle as po

SKELETONS = (po.MEDIAPIPE, po.NTU)


def case_names(fx):
    return [str(n) for n in fx["case_names"]]


def case(fx, name):
    W, stride, skel = (int(v) for v in fx[f"{name}_cfg"])
    return fx[f"{name}_seq"], fx[f"{name}_table"], W, stride, SKELETONS[skel]


def fixture_intervals(fx, name):
    return [{"start_frame": int(f[0]), "end_frame": int(f[1]), "start_time": str(t[0]),
             "end_time": str(t[1]), "mean_confidence": float(c[0]),
             "peak_confidence": float(c[1]), "peak_frame": int(f[2])}
            for f, c, t in zip(fx[f"{name}_iv_frames"], fx[f"{name}_iv_conf"],
                               fx[f"{name}_iv_times"])]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pipeline_fixtures.npz")


@pytest.fixture(scope="module")
def ref32(golden):
    return golden("pipeline_fixtures_ref32.npz")


def test_fixture_cases_present(fx, ref32):
    names = case_names(fx)
    assert len(names) == 14 and "w300" in names and "ntu_empty" in names
    # the edge cases the fixtures exist for
    assert fx["short_table"].tolist() == [[0, 20]]
    assert fx["exact96_table"].tolist() == [[0, 48], [24, 48], [48, 48]]
    assert fx["exact72_table"].tolist() == [[0, 48], [24, 48]]
    assert fx["plain_table"].tolist()[-1] == [96, 35]
    assert not ref32["allnull_ref32"][2].any() and ref32["allnull_ref32"][1].any()


def test_normalize_bit_exact_against_reference(fx, ref32):
    for name in case_names(fx):
        seq, table, W, stride, skel = case(fx, name)
        got = po.normalize_windows(seq, table, W, skel)
        assert got.dtype == np.float32
        assert np.array_equal(got, ref32[f"{name}_ref32"]), name


def test_normalize_fp64_mode(golden, fx, ref32):
    f64 = golden("pipeline_fixtures_f64.npz")
    for name in case_names(fx):
        seq, table, W, stride, skel = case(fx, name)
        ref64 = ref32[f"{name}_ref32"].astype(np.float64) + f64[f"{name}_d64"]
        got = po.normalize_windows(seq, table, W, skel, fp64=True)
        assert got.dtype == np.float64
        # the stored difference is rounded to float32: ~1e-14 on values of order 1
        assert np.abs(got - ref64).max() <= 1e-12, name


def test_stages_are_prefixes_of_the_chain(fx):
    """stages=1 only moves frames; stages=3 is stages=1 centred; a plain window (no null
    frame) is its own stage 1."""
    seq, table, W, stride, skel = case(fx, "nullruns")
    s1 = po.normalize_windows(seq, table, W, skel, stages=1)
    raw = po.cut_windows(seq, table, W)
    # window 4 = frames 96..130: 96..109 null, 110..124 real, 125..130 null, then the padding
    real = raw[4, :, 14:29]
    assert np.array_equal(s1[4, :, :15], real)
    assert np.array_equal(s1[4, :, 15:], np.concatenate([real] * 3, 1)[:, :33])
    # window 1 = frames 24..71: 30..32 null in the middle stay zero, 60..71 null: L = 36
    assert np.array_equal(s1[1, :, :36], raw[1, :, :36]) and not s1[1, :, 6:9].any()
    assert np.array_equal(s1[1, :, 36:], raw[1, :, :12])
    assert np.array_equal(s1[0, :, :25], raw[0, :, [*range(5, 30)]].transpose(1, 0, 2, 3))
    s3 = po.normalize_windows(seq, table, W, skel, stages=3)
    hip = (s1[:, :, :, 23, 0] + s1[:, :, :, 24, 0]) / np.float32(2)
    assert np.array_equal(s3[:, :, :, 5, 0], s1[:, :, :, 5, 0] - hip)
    seq, table, W, stride, skel = case(fx, "plain")
    assert np.array_equal(po.normalize_windows(seq, table, W, skel, stages=1)[:4],
                          po.cut_windows(seq, table, W)[:4])


def test_source_map_small_cases():
    f = lambda bits: po.source_map(np.array(bits, dtype=bool)).tolist()   # noqa: E731
    assert f([0, 0, 0, 0]) == [-1, -1, -1, -1]
    assert f([1, 0, 0, 0]) == [0, 0, 0, 0]                       # L = 1
    assert f([1, 1, 0, 1, 0, 0, 0, 0, 0]) == [0, 1, -1, 3, 0, 1, -1, 3, 0]
    assert f([0, 1, 0, 1, 1, 0]) == [1, 3, 4, 1, 3, 4]           # compacted, then filled
    assert f([1, 1, 1]) == [0, 1, 2]


@pytest.mark.parametrize("table_fn", ["oracle", "product"])
def test_window_table(fx, table_fn):
    if table_fn == "oracle":
        fn = po.sliding_window_table
    else:
        from shiftgcn import pipeline
        fn = pipeline.sliding_window_table
    for name in case_names(fx) + ["e2e"]:
        W, stride, _ = (int(v) for v in fx[f"{name}_cfg"])
        got = fn(fx[f"{name}_seq"].shape[1], W, stride)
        assert got.dtype == np.int32 and np.array_equal(got, fx[f"{name}_table"]), name
    assert fn(1, 300, 150).tolist() == [[0, 1]]
    assert fn(301, 300, 150).tolist() == [[0, 300], [150, 151]]
    assert fn(450, 300, 150).tolist() == [[0, 300], [150, 300]]


def test_aggregate_bit_exact(fx):
    for name in case_names(fx) + ["e2e"]:
        T = fx[f"{name}_seq"].shape[1]
        got = po.aggregate_per_frame(fx[f"{name}_scores"], fx[f"{name}_table"], T)
        assert np.array_equal(got, fx[f"{name}_per_frame"]), name


@pytest.mark.parametrize("impl", ["oracle", "product"])
def test_fall_intervals(fx, impl):
    if impl == "oracle":
        fn = po.detect_fall_intervals
    else:
        from shiftgcn import pipeline
        fn = pipeline.detect_fall_intervals
    fps = float(fx["fps"])
    for name in case_names(fx) + ["e2e"]:
        thr = float(fx["e2e_threshold"]) if name == "e2e" else 0.5
        assert fn(fx[f"{name}_per_frame"], thr, fps) == fixture_intervals(fx, name), name
    assert fn(np.zeros(7), 0.5, fps) == []
    one = fn(np.array([0.9, 0.7]), 0.5, 0.5)[0]                   # 2 frames at 0.5 fps
    assert (one["start_time"], one["end_time"], one["peak_frame"]) == ("0:00.00", "0:04.00", 0)
    assert fn(np.linspace(0, 1, 4000), 0.5, 30.0)[0]["end_time"] == "2:13.33"
