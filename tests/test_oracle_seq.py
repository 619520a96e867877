"""The case tables of the sequence and modality kernels (oracle/seq_cases.py): the
``sgcn_window_normalize`` table reaches every branch of the tag universe, every case's
declared tags are the ones computed from its inputs, and the numpy closed form
(tests/pipeline_oracle.py) is bit-equal to the reference's own ``pre_normalize`` /
``pre_normalization`` on every case (tests/golden/seq_fixtures.npz, made by
gen_seq_fixtures.py): the oracle's pin, extended to the degenerate branches. No GPU."""
import math

import numpy as np
import pytest

import pipeline_oracle as po
from oracle import ensemble_oracle as eo
from oracle import seq_cases as sc


@pytest.fixture(scope="module")
def fx(golden):
    return golden("seq_fixtures.npz")


def test_table_reaches_the_tag_universe():
    reached = set().union(*(sc.tags(c) for c in sc.CASES))
    assert reached == sc.TAG_UNIVERSE, (sc.TAG_UNIVERSE - reached, reached - sc.TAG_UNIVERSE)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_declared_tags_are_the_computed_ones(name):
    case = sc.BY_NAME[name]
    got = sc.tags(case)
    assert got == case["tags"], (sorted(got - case["tags"]), sorted(case["tags"] - got))


def test_size_rules():
    assert all(c["V"] == 4 for c in sc.CASES if c["W"] > 300)
    assert all(len(c["table"]) <= 3 and c["W"] * c["M"] <= 2048 for c in sc.CASES)
    production = [c for c in sc.CASES if (c["W"], c["V"], c["M"]) == (300, 25, 2)]
    assert len(production) == 1 and len(production[0]["table"]) == 1
    # a host table as the product would accept it, and some frame outside every row
    for c in sc.CASES:
        assert sc.clamped_rows(c) == [tuple(r) for r in c["table"].tolist()], c["name"]
    assert any(_uncovered(c).any() for c in sc.CASES)


def _uncovered(case):
    free = np.ones(case["T"], dtype=bool)
    for s, r in case["table"]:
        free[s:s + r] = False
    return free


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_rotations_are_well_conditioned(name):
    """Under every stage mask that rotates: a general rotation has its angle in
    [0.2, pi - 0.2], and on a case compared in error-bar form the float64 oracle takes the
    float32 oracle's branch for every rotation."""
    case = sc.BY_NAME[name]
    for stages in sc.ROTATING:
        k32 = sc.windows_kinds(case, stages=stages)
        k64 = sc.windows_kinds(case, fp64=True, stages=stages)
        for w32, w64 in zip(k32, k64):
            for (kind, angle), (kind64, _) in zip(w32, w64):
                if kind == "general":
                    assert 0.2 <= angle <= math.pi - 0.2, (name, stages, angle)
                if not sc.all_identity(case, stages):
                    assert kind64 == kind, (name, stages, kind, kind64)


def test_fixture_holds_results_only(fx):
    want = {"case_names"} | {f"{n}_ref32" for n in sc.CASE_NAMES} | \
        {f"{c['name']}_d64" for c in sc.CASES if not sc.all_identity(c)}
    assert set(fx.files) == want
    assert [str(n) for n in fx["case_names"]] == sc.CASE_NAMES


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_bit_equal_to_reference(fx, name):
    case = sc.BY_NAME[name]
    got = po.normalize_windows(sc.build(name), case["table"], case["W"],
                               sc.SKELETONS[case["skel"]])
    assert got.dtype == np.float32
    assert np.array_equal(got, fx[f"{name}_ref32"])


@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES if not sc.all_identity(c)])
def test_oracle_fp64_mode(fx, name):
    case = sc.BY_NAME[name]
    ref64 = fx[f"{name}_ref32"].astype(np.float64) + fx[f"{name}_d64"]
    got = po.normalize_windows(sc.build(name), case["table"], case["W"],
                               sc.SKELETONS[case["skel"]], fp64=True)
    assert got.dtype == np.float64
    # the stored difference is rounded to float32: ~1e-14 on values of order 1
    assert np.abs(got - ref64).max() <= 1e-12


def test_cancelling_joint_stays_zero(fx):
    """The joints of mp_cancel whose values cancel are not zero going in and zero coming
    out, through centring and both rotations."""
    seq = sc.build("mp_cancel")
    out = fx["mp_cancel_ref32"][0]
    for t, v in ((1, 5), (3, 5), (0, 30), (2, 24)):
        assert seq[:, t, v, 0].any() and not out[:, t, v, 0].any()


def test_aggregate_cases():
    names = [c["name"] for c in sc.AGG_CASES]
    assert {c["total_frames"] for c in sc.AGG_CASES} >= {1, 255, 256, 257, 600}
    for c in sc.AGG_CASES:
        depth, F, rows = sc.agg_depths(c), c["total_frames"], c["table"].tolist()
        if c["name"].startswith("F") and F > 1:
            assert {0, 1, 5} <= set(depth.tolist()), c["name"]
            assert any(r == 0 for _, r in rows) and len(set(map(tuple, rows))) < len(rows)
            assert any(a[0] > b[0] for a, b in zip(rows, rows[1:]))         # out of order
            assert any(s + r > F for s, r in rows) and any(s + r == F for s, r in rows)
    order = sc.AGG_CASES[names.index("table_order")]
    in_order = po.aggregate_per_frame(sc.agg_scores(order), order["table"], 7)
    assert in_order.tolist() == [0.0] + [0.25] * 5 + [0.0]
    swapped = sc.agg_scores(order)[[0, 2, 1, 3]]
    assert po.aggregate_per_frame(swapped, order["table"], 7)[1] == 0.5
    empty = sc.AGG_CASES[names.index("empty_table")]
    assert (empty["total_frames"], len(empty["table"])) == (9, 0)


def test_modality_cases():
    shapes = [s for s, _, _ in sc.MOD_CASES]
    totals = [int(np.prod(s)) for s in shapes]
    assert 256 in totals and 257 in totals
    assert {(1, 3, 1, 25, 2), (2, 3, 5, 33, 1), (1, 3, 7, 25, 2), (1, 2, 4, 8, 2),
            (1, 5, 3, 4, 2)} <= set(shapes)
    assert all(bn for s, _, bn in sc.MOD_CASES if s[4] == 2 and int(np.prod(s)) != 256)
    par = sc.synthetic_parents(8)
    assert par[0] == 0 and (par[1:4] > np.arange(1, 4)).all()
    # the parent-table form of the oracle is the bone-pair form
    joint, _, _ = sc.mod_inputs((1, 2, 4, 8, 2))
    a = eo.derive_modalities(joint, parent=par)
    b = eo.derive_modalities(joint, list(enumerate(par.tolist())))
    assert all(np.array_equal(a[s], b[s]) for s in eo.MODALITIES)
    assert not a["bone"][..., 0, :].any() and a["bone"][..., 1, :].any()
    f = sc.data_bn_feature((1, 2, 4, 8, 2))
    assert f.shape == (2, 2, 4, 8) and f[1, 1, 3, 5] == (1 * 8 + 5) * 2 + 1
