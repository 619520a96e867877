"""The sequence and modality kernels (sequence.hip: window_normalize_kernel,
window_aggregate_kernel; ensemble.hip: modalities_kernel) through their raw ABI, against the
numpy closed forms (tests/pipeline_oracle.py, oracle/ensemble_oracle.py) and the reference's
own outputs (tests/golden/seq_fixtures.npz) at every branch.

The cases (oracle/seq_cases.py) are the smallest that reach each branch of the source-frame
map and its multi-chunk block scan, the null test, the centre, every identity branch of the
two rotations and the ABI limit W*M = 2048; tests/test_oracle_seq.py checks that coverage,
and pins the closed form to the reference on every case, without a GPU.

Every operand is laid into a poisoned allocation: inputs sit in NaN, outputs between margins
of a sentinel bit pattern that must survive bit for bit. ``window_normalize`` runs once more
per case with every frame that no table row covers set to NaN, and must give the same bits.

Bars (DESIGN.md "Parity bars"):
  window_normalize stages 0..3 (pad, centre)      equal to the closed form;
  stages 4..7 where every rotation is the identity equal to the closed form, and stage 7 to
                                                  the reference fixture;
  stages 4..7 otherwise                           the zero pattern of the float32 reference,
      and max|got - ref64| <= 2 x max|ref32 - ref64| (stage 7: the reference fixture's two
      results; stages 4..6, which the reference cannot run: the closed form's two precisions);
  window_aggregate, the four streams              equal to the closed form;
  data_bn   |got - (x*s + b)| <= 1.01 * 2^-24 * (|x*s| + |x*s + b|), the product and the sum
            in float64: one rounding of the product and one of the sum, or one of the fused
            form (the file does not forbid contraction).
Each error-bar figure is printed before it is asserted.

Measured on an MI355X (93 cases, 3 s): every error-bar case of window_normalize sits at
0.500 of its bar, bit-equal to the float32 reference (worst absolute figure 3.93e-7 at
mp_cancel stages 6 and 7, against the same 3.93e-7 from the float32 reference); data_bn at most 1.2e-7 / 0.845 of its bound (1x3x7x25x2, bone). Before |v| of a
rotation's bone rounded its sum of squares once, as numpy's float32 dot product does, t4_w256
at stage 5 was at 2.87e-7 against 1.37e-7, 1.043 of its bar.
"""
import functools

import numpy as np
import pytest
import torch

import pipeline_oracle as po
from oracle import ensemble_oracle as eo
from oracle import seq_cases as sc
from test_gpu_pw_ref import SENTINEL

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 64                                   # elements on either side of an operand


def _in_nan(data):
    """A float32 operand inside a NaN-filled allocation; (allocation, operand view)."""
    flat = torch.from_numpy(np.array(data, dtype=np.float32).reshape(-1))
    buf = torch.full((flat.numel() + 2 * MARGIN,), float("nan"), device=DEV)
    buf[MARGIN:MARGIN + flat.numel()] = flat.to(DEV)
    return buf, buf[MARGIN:MARGIN + flat.numel()]


def _in_sentinel(n, dtype=torch.float32):
    """An n-element output between two sentinel margins; (allocation, output view)."""
    buf = torch.empty(n + 2 * MARGIN, device=DEV, dtype=dtype)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf[MARGIN:MARGIN + n]


def _margins_intact(buf, n):
    words = buf.element_size() // 4
    m = buf.view(torch.int32)
    return bool((m[:MARGIN * words] == SENTINEL).all()
                and (m[(MARGIN + n) * words:] == SENTINEL).all())


def _all_written(view):
    """No element of a float32 output still holds the sentinel."""
    return not bool((view.view(torch.int32) == SENTINEL).any())


def _lib():
    from shiftgcn import _lib as lib
    return lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------------------
# sgcn_window_normalize
# --------------------------------------------------------------------------------------
def _normalize(case, stages, poison=False):
    """The kernel's (n, 3, W, V, M) output for a case; ``poison`` sets every frame that no
    table row covers to NaN."""
    seq = sc.build(case["name"])
    if poison:
        seq = seq.copy()
        free = np.ones(case["T"], dtype=bool)
        for s, r in sc.clamped_rows(case):
            free[s:s + r] = False
        seq[:, free] = np.nan
    W, V, M, T, n = case["W"], case["V"], case["M"], case["T"], len(case["table"])
    sk = sc.SKELETONS[case["skel"]]
    seq_buf, d_seq = _in_nan(seq)
    total = n * 3 * W * V * M
    out_buf, d_out = _in_sentinel(total)
    table = torch.from_numpy(case["table"]).to(DEV)
    rc = _lib().sgcn_window_normalize(
        d_seq.data_ptr(), table.data_ptr(), d_out.data_ptr(), n, T, V, M, W,
        sk["zaxis"][0], sk["zaxis"][1], sk["xaxis"][0], sk["xaxis"][1], sk["center"][0],
        sk["center"][1] if len(sk["center"]) == 2 else -1, stages, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    what = f"{case['name']} stages {stages}"
    assert _margins_intact(out_buf, total), f"{what}: a store outside the output"
    assert _all_written(d_out), f"{what}: an output element was not written"
    assert torch.equal(table.cpu(), torch.from_numpy(case["table"]))
    return d_out.cpu().numpy().reshape(n, 3, W, V, M)


@functools.lru_cache(maxsize=None)
def _oracle(name, stages, fp64=False):
    case = sc.BY_NAME[name]
    out = po.normalize_windows(sc.build(name), case["table"], case["W"],
                               sc.SKELETONS[case["skel"]], stages=stages, fp64=fp64)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def fx(golden):
    return golden("seq_fixtures.npz")


def _error_bar(got, ref32, ref64, what):
    """The zero pattern of the float32 reference, and no further from the float64 one than
    twice the float32 one is. Returns the share of the bar used."""
    assert np.array_equal(got == 0, ref32 == 0), f"{what}: zero pattern"
    ref_err = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    used = err / (2 * ref_err)
    print(f"{what}: max|ours - ref64| = {err:.3e}, max|ref32 - ref64| = {ref_err:.3e}, "
          f"bar use {used:.3f}")
    assert err <= 2 * ref_err, (what, err, ref_err)
    return used


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_normalize_pad_and_centre_exact(name):
    case = sc.BY_NAME[name]
    for stages in (0, 1, 2, 3):
        got = _normalize(case, stages)
        assert np.array_equal(got, _oracle(name, stages)), (name, stages)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_normalize_rotation_prefixes(name):
    """Stages 4, 5 and 6 (rotation without the padding, the centring or both)."""
    case = sc.BY_NAME[name]
    for stages in (4, 5, 6):
        got = _normalize(case, stages)
        if sc.all_identity(case, stages):
            assert np.array_equal(got, _oracle(name, stages)), (name, stages)
        else:
            _error_bar(got, _oracle(name, stages), _oracle(name, stages, True),
                       f"{name} stages {stages}")


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_normalize_against_reference(fx, name):
    case = sc.BY_NAME[name]
    got = _normalize(case, 7)
    ref32 = fx[f"{name}_ref32"]
    if sc.all_identity(case):
        # an identity matrix applied in float64 and rounded is exact
        assert np.array_equal(got, ref32), name
    else:
        ref64 = ref32.astype(np.float64) + fx[f"{name}_d64"]
        _error_bar(got, ref32, ref64, f"{name} stages 7")


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_normalize_reads_no_uncovered_frame(name):
    """With NaN in every frame outside the table's rows the output keeps its bits."""
    case = sc.BY_NAME[name]
    for stages in (3, 7):
        clean = _normalize(case, stages)
        poisoned = _normalize(case, stages, poison=True)
        assert np.array_equal(clean.view(np.int32), poisoned.view(np.int32)), (name, stages)


# --------------------------------------------------------------------------------------
# sgcn_window_aggregate
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.AGG_CASES, ids=lambda c: c["name"])
def test_aggregate_exact(case):
    F, n = case["total_frames"], len(case["table"])
    scores = sc.agg_scores(case)
    want = po.aggregate_per_frame(scores, case["table"], F)
    d_scores = torch.from_numpy(scores).to(DEV) if n else None
    d_table = torch.from_numpy(case["table"]).to(DEV) if n else None
    buf, per_frame = _in_sentinel(F, torch.float64)
    rc = _lib().sgcn_window_aggregate(
        d_scores.data_ptr() if n else None, d_table.data_ptr() if n else None,
        per_frame.data_ptr(), n, F, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _margins_intact(buf, F), "a store outside per_frame"
    got = per_frame.cpu().numpy()
    assert np.array_equal(got, want), case["name"]
    if case["name"] == "table_order":
        assert got[1] == 0.25
    if case["name"] == "empty_table":
        assert got.tolist() == [0.0] * 9


# --------------------------------------------------------------------------------------
# sgcn_modalities
# --------------------------------------------------------------------------------------
def _parents(kind, V):
    from shiftgcn import ensemble as ens
    if kind == "syn":
        return sc.synthetic_parents(V)
    pairs = ens.NTU_BONE_PAIRS if kind == "ntu" else ens.MEDIAPIPE_BONE_PAIRS
    return ens.parent_table(pairs, V)


def _modalities(shape, joint, parent, planes, which=(0, 1, 2, 3), scale=None, shift=None):
    """The outputs ``which`` of one launch (the others NULL), as numpy; None for a NULL."""
    N, C, T, V, M = shape
    total = int(np.prod(shape))
    joint_buf, d_joint = _in_nan(joint)
    d_parent = torch.from_numpy(parent).to(DEV)
    outs = [_in_sentinel(total) if k in which else None for k in range(4)]
    coef = [None if a is None else torch.from_numpy(a).to(DEV) for a in (scale, shift)]
    rc = _lib().sgcn_modalities(
        d_joint.data_ptr(), d_parent.data_ptr(),
        *[None if o is None else o[1].data_ptr() for o in outs],
        *[None if a is None else a.data_ptr() for a in coef],
        int(planes), N, C, T, V, M, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert _margins_intact(o[0], total), "a store outside an output"
            assert _all_written(o[1]), "an output element was not written"
    assert torch.equal(joint_buf[MARGIN:MARGIN + total].cpu(),
                       torch.from_numpy(joint.reshape(-1)))
    out_shape = (N * M, C, T, V) if planes else shape
    return [None if o is None else o[1].cpu().numpy().reshape(out_shape) for o in outs]


def _mod_id(case):
    return "x".join(map(str, case[0])) + "-" + case[1]


@pytest.mark.parametrize("planes", [0, 1])
@pytest.mark.parametrize("case", sc.MOD_CASES, ids=_mod_id)
def test_modalities_exact(case, planes):
    shape, kind, _ = case
    joint, _, _ = sc.mod_inputs(shape)
    parent = _parents(kind, shape[3])
    ref = eo.derive_modalities(joint, parent=parent)
    if shape[2] == 1:
        assert not ref["joint_motion"].any() and not ref["bone_motion"].any()
    four = _modalities(shape, joint, parent, planes)
    for k, s in enumerate(eo.MODALITIES):
        want = sc.to_planes(ref[s]) if planes else ref[s]
        assert np.array_equal(four[k], want), s
        # alone, with the other three NULL: the same bits
        alone = _modalities(shape, joint, parent, planes, which=(k,))
        assert [a is None for a in alone] == [i != k for i in range(4)]
        assert np.array_equal(alone[k].view(np.int32), four[k].view(np.int32)), s


@pytest.mark.parametrize("case", [c for c in sc.MOD_CASES if c[2]], ids=_mod_id)
def test_modalities_data_bn(case):
    shape, kind, _ = case
    joint, scale, shift = sc.mod_inputs(shape)
    parent = _parents(kind, shape[3])
    ref = eo.derive_modalities(joint, parent=parent)
    feat = sc.data_bn_feature(shape)
    four = _modalities(shape, joint, parent, 1, scale=scale, shift=shift)
    worst = 0.0
    for k, s in enumerate(eo.MODALITIES):
        x = sc.to_planes(ref[s]).astype(np.float64)
        xs = x * scale[k].astype(np.float64)[feat]
        want = xs + shift[k].astype(np.float64)[feat]
        bar = 1.01 * 2.0 ** -24 * (np.abs(xs) + np.abs(want))
        err = np.abs(four[k].astype(np.float64) - want)
        used = float((err / np.maximum(bar, np.finfo(np.float64).tiny)).max())
        worst = max(worst, used)
        print(f"data_bn {_mod_id(case)} {s}: max err {float(err.max()):.3e}, bar use {used:.3f}")
        assert (err <= bar).all(), (s, float(err.max()), used)
        alone = _modalities(shape, joint, parent, 1, which=(k,), scale=scale, shift=shift)
        assert np.array_equal(alone[k].view(np.int32), four[k].view(np.int32)), s
    print(f"data_bn {_mod_id(case)}: worst bar use {worst:.3f}")
