"""Case tables of the sequence and modality kernels (``csrc/sequence.hip``,
``csrc/ensemble.hip``) and the branches each ``sgcn_window_normalize`` case reaches
(TEST INFRASTRUCTURE ONLY; no GPU, and no torch before a sequence is built).

A ``window_normalize`` case is a name, ``W``, ``V``, ``M``, a skeleton, a sequence recipe
(``tests/golden/formula.py`` seeds plus explicit edits, as ``gen_pipeline_fixtures.py``
does) and a window table; the inputs are regenerated from the recipe (:func:`build`), never
stored. :func:`tags` restates, from ``tests/pipeline_oracle.py`` (``source_map``,
``align_angle``, the null flags), which branches of the kernel a case reaches, per window and
per person; every case declares its tags and ``tests/test_oracle_seq.py`` checks the
declaration, and that the table reaches the whole of :data:`TAG_UNIVERSE`.

Shapes are the smallest that carry their tag: ``V = 4`` (the test skeleton ``T4``) above
``W = 300``, at most three windows per case, and the NTU production shape
``W = 300, V = 25, M = 2`` once, with one window. The windows above ``W = 300`` keep few
source frames, so that their (periodic) reference outputs compress.

A rotation declared ``general`` has its angle in [0.2, pi - 0.2] by the oracle (the seed of
a case is searched, as the pipeline fixtures' is), and on a case compared in error-bar form
the float64 oracle takes the same branch as the float32 one for every rotation: conditions
on the inputs, asserted on the CPU.
"""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_REPO, "tests"), os.path.join(_REPO, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pipeline_oracle as po  # noqa: E402

T4 = dict(zaxis=(0, 1), xaxis=(2, 3), center=(1,))
SKELETONS = {"mp": po.MEDIAPIPE, "ntu": po.NTU, "t4": T4}
ROT_KINDS = ("general", "identity_l1", "identity_axis_parallel", "identity_axis_antiparallel",
             "identity_theta", "axis_joint_absent_frame0")
TAG_UNIVERSE = frozenset(
    [f"map:{t}" for t in ("absent", "plain_full", "wrap_once", "wrap_many", "L1",
                          "interior_null_before_L", "compact", "compact_count1",
                          "compact_only_first_null")]
    + [f"scan:{t}" for t in ("one_chunk", "W256", "W257", "two_chunks_M2",
                             "compact_straddles_256", "survivors_only_in_chunk1",
                             "survivor_on_each_wave_boundary", "WM_at_limit_M1",
                             "WM_at_limit_M2")]
    + [f"table:{t}" for t in ("start_gt0", "tail_window", "nr0", "compact_in_nonfirst_window")]
    + [f"null:{t}" for t in ("nonnull_by_last_z_only", "negzero_frame_is_null",
                             "p0_null_p1_not_same_frame", "p0_absent_p1_present")]
    + [f"centre:{t}" for t in ("one_joint", "two_joint", "centre_frame_zero_while_p1_present",
                               "joint_absent_by_cancellation")]
    + [f"rot_{a}:{k}" for a in "zx" for k in ROT_KINDS])


# --------------------------------------------------------------------------------------
# sequence recipes
# --------------------------------------------------------------------------------------
def sequence(seed, T, V, M):
    """A pose (one value per channel and joint, scale 1) plus per-frame motion: the
    sequences of ``gen_pipeline_fixtures.py``."""
    import formula
    pose = formula.tensor((3, 1, V, 1), seed, 1.0).numpy()
    move = formula.tensor((3, T, V, M), seed + 1, 0.25).numpy()
    shift = formula.tensor((3, 1, 1, M), seed + 2, 0.5).numpy()
    return (pose + move + shift).astype(np.float32)


def _frames(spec):
    """Frame numbers of a list of ints and (first, stop[, step]) ranges."""
    out = []
    for s in spec:
        out.extend(range(*s) if isinstance(s, tuple) else [s])
    return out


def apply_edit(seq, edit):
    """One edit of a recipe, in place:
    ("null", frames, person)     the frames of a person (None: everyone) become 0;
    ("keep", frames, person)     every other frame of the person becomes 0;
    ("negzero", frames, person)  the frames become -0.0 in every value;
    ("lastz", frames, person, z) the frames become 0 but for the last joint's z;
    ("joint", t, v, m, xyz)      one joint is set."""
    op = edit[0]
    if op == "joint":
        _, t, v, m, xyz = edit
        seq[:, t, v, m] = np.asarray(xyz, dtype=np.float32)
        return
    frames, m = _frames(edit[1]), edit[2]
    who = slice(None) if m is None else m
    if op == "keep":
        drop = np.ones(seq.shape[1], dtype=bool)
        drop[frames] = False
        frames = np.flatnonzero(drop)
    seq[:, frames, :, who] = -0.0 if op == "negzero" else 0.0
    if op == "lastz":
        seq[2, frames, -1, who] = edit[3]


def _case(name, skel, W, V, M, T, table, edits, tags):
    assert V == {"mp": 33, "ntu": 25, "t4": 4}[skel] and len(table) <= 3
    return dict(name=name, skel=skel, W=W, V=V, M=M, T=T,
                table=np.array(table, dtype=np.int32).reshape(-1, 2), edits=tuple(edits),
                tags=frozenset(tags))


def _rot(z, x):
    z, x = ([k] if isinstance(k, str) else k for k in (z, x))
    return [f"rot_z:{k}" for k in z] + [f"rot_x:{k}" for k in x]


_PLAIN = ["map:plain_full", "scan:one_chunk"]
_ABS0 = "axis_joint_absent_frame0"

# frame-0 joints of the T4 skeleton (person 0) whose bones are exact in float32. Joint 1 is
# the centre and the top of the z bone, so the z bone is j1 - j0 and the x bone j2 - j3.
_J1 = (0.5, 0.25, 1.0)


def _t4_frame0(t, j0, j2, j3):
    return [("joint", t, 1, 0, _J1), ("joint", t, 0, 0, j0), ("joint", t, 2, 0, j2),
            ("joint", t, 3, 0, j3)]


CASES = [
    _case("mp_plain", "mp", 12, 33, 1, 12, [[0, 12]], [],
          _PLAIN + ["centre:two_joint"] + _rot("general", "general")),
    # frames 10, 11 null: window 0 wraps once at L = 10, window 1 starts on a null frame,
    # window 2 is a tail of 6; frame 30 is outside every row
    _case("mp_table", "mp", 12, 33, 1, 31, [[0, 12], [10, 12], [24, 6]],
          [("null", [10, 11], None)],
          ["scan:one_chunk", "map:wrap_once", "map:compact", "table:start_gt0",
           "table:tail_window", "table:compact_in_nonfirst_window", "centre:two_joint"]
          + _rot("general", "general")),
    # cancelling joints (1.5 - 0.5 - 1.0) in frames whose sums stay non-zero
    _case("mp_cancel", "mp", 6, 33, 1, 6, [[0, 6]],
          [("joint", 1, 5, 0, (1.5, -0.5, -1.0)), ("joint", 3, 5, 0, (1.5, -0.5, -1.0)),
           ("joint", 0, 30, 0, (-2.0, 0.75, 1.25)), ("joint", 2, 24, 0, (0.25, 0.25, -0.5))],
          _PLAIN + ["centre:two_joint", "centre:joint_absent_by_cancellation"]
          + _rot("general", "general")),
    # joint 11 (top of the z bone, left end of the x bone) absent in frame 0
    _case("mp_axis0", "mp", 6, 33, 1, 7, [[1, 6]],
          [("joint", 1, 11, 0, (0.0, 0.0, 0.0))],
          _PLAIN + ["table:start_gt0", "centre:two_joint"]
          + _rot(["general", _ABS0], ["general", _ABS0])),
    # person 0 has a null frame 4 inside its run while person 1 is there; a second row of
    # length 0
    _case("ntu_people", "ntu", 10, 25, 2, 10, [[0, 10], [2, 0]],
          [("null", [4, 8, 9], 0), ("null", [9], 1)],
          ["scan:one_chunk", "map:interior_null_before_L", "map:wrap_once", "map:absent",
           "table:start_gt0", "table:nr0", "null:p0_null_p1_not_same_frame",
           "centre:one_joint", "centre:centre_frame_zero_while_p1_present"]
          + _rot("general", "general")),
    # person 0 absent; person 1 null in frame 0 only
    _case("ntu_p0absent", "ntu", 6, 25, 2, 6, [[0, 6]],
          [("null", [(0, 6)], 0), ("null", [0], 1)],
          ["scan:one_chunk", "map:absent", "map:compact", "map:compact_only_first_null",
           "map:wrap_once", "null:p0_absent_p1_present", "null:p0_null_p1_not_same_frame",
           "centre:one_joint", "centre:centre_frame_zero_while_p1_present"]
          + _rot(["identity_l1", _ABS0], ["identity_l1", _ABS0])),
    # one real frame repeated: frame 0 for person 0, frame 3 (compacted) for person 1
    _case("t4_L1", "t4", 7, 4, 2, 7, [[0, 7]],
          [("keep", [0], 0), ("keep", [3], 1)],
          ["scan:one_chunk", "map:L1", "map:wrap_many", "map:compact", "map:compact_count1",
           "null:p0_null_p1_not_same_frame", "centre:one_joint"]
          + _rot("general", "general")),
    # frames 0, 1, 3 real: L = 4, three and a quarter periods
    _case("t4_wrapmany", "t4", 13, 4, 1, 13, [[0, 13]],
          [("keep", [0, 1, 3], 0)],
          ["scan:one_chunk", "map:wrap_many", "map:interior_null_before_L",
           "centre:one_joint"] + _rot("general", "general")),
    # person 0: frames 0 and 4 non-null through the last joint's z alone, 5.. null;
    # person 1: frame 0 and frame 5 are -0.0 everywhere, 6.. null
    _case("t4_nulltest", "t4", 8, 4, 2, 8, [[0, 8]],
          [("lastz", [0, 4], 0, 0.75), ("null", [(5, 8)], 0),
           ("negzero", [0, 5], 1), ("null", [6, 7], 1)],
          ["scan:one_chunk", "map:wrap_once", "map:compact", "map:compact_only_first_null",
           "null:nonnull_by_last_z_only", "null:negzero_frame_is_null", "centre:one_joint"]
          + _rot(["identity_l1", _ABS0], ["general", _ABS0])),
    # three windows whose frame 0 makes both rotations the identity: z bone along +z and
    # x bone along -x; z bone along -z and x bone along +x; cosines that round to 1
    _case("t4_identity", "t4", 5, 4, 1, 15, [[0, 5], [5, 5], [10, 5]],
          _t4_frame0(0, (0.5, 0.25, 0.5), (0.5, 0.5, 2.0), (1.0, 0.5, 2.0))
          + _t4_frame0(5, (0.5, 0.25, 1.5), (1.0, 0.5, 2.0), (0.5, 0.5, 2.0))
          + _t4_frame0(10, (0.5 - 1e-5, 0.25, 0.0), (1.0, 0.5 + 1e-5, 2.0), (0.0, 0.5, 2.0)),
          _PLAIN + ["table:start_gt0", "centre:one_joint"]
          + _rot(["identity_axis_parallel", "identity_axis_antiparallel", "identity_theta"],
                 ["identity_axis_parallel", "identity_axis_antiparallel", "identity_theta"])),
    # one identity and one general rotation: equal x joints under a general z rotation,
    # then a z bone along +z with a general x bone
    _case("t4_mixed", "t4", 5, 4, 1, 10, [[0, 5], [5, 5]],
          [("joint", 0, 3, 0, (0.375, -0.5, 0.25)), ("joint", 0, 2, 0, (0.375, -0.5, 0.25)),
           ("joint", 5, 1, 0, _J1), ("joint", 5, 0, 0, (0.5, 0.25, 0.5))],
          _PLAIN + ["table:start_gt0", "centre:one_joint"]
          + _rot(["general", "identity_axis_parallel"], ["identity_l1", "general"])),
    # an exactly full chunk; compacted, with a null run inside
    _case("t4_w256", "t4", 256, 4, 1, 256, [[0, 256]],
          [("null", [0, (100, 110), (200, 256)], 0)],
          ["scan:one_chunk", "scan:W256", "map:compact", "map:wrap_once",
           "centre:one_joint"] + _rot("general", "general")),
    # a second chunk of one thread, and that frame is a survivor of a compaction
    _case("t4_w257", "t4", 257, 4, 1, 257, [[0, 257]],
          [("null", [(0, 3), (250, 256)], 0)],
          ["scan:W257", "scan:compact_straddles_256", "map:compact", "map:wrap_once",
           "centre:one_joint"] + _rot("general", "general")),
    # person 0: survivors 64..127 and 192..289 (flags differ across 63/64, 127/128, 191/192);
    # person 1: survivors 260..279 only
    _case("t4_w300", "t4", 300, 4, 2, 302, [[1, 300]],
          [("keep", [(65, 129), (193, 291)], 0), ("keep", [(261, 281)], 1)],
          ["scan:two_chunks_M2", "scan:compact_straddles_256",
           "scan:survivors_only_in_chunk1", "scan:survivor_on_each_wave_boundary",
           "map:compact", "map:wrap_once", "map:wrap_many", "table:start_gt0",
           "centre:one_joint"] + _rot("general", "general")),
    # the NTU production shape, once: person 0 keeps 60 frames with a hole, person 1 is
    # compacted from both sides of frame 256
    _case("ntu_w300", "ntu", 300, 25, 2, 300, [[0, 300]],
          [("keep", [(0, 20), (24, 60)], 0), ("keep", [(250, 270)], 1)],
          ["scan:two_chunks_M2", "scan:compact_straddles_256", "map:compact",
           "map:wrap_many", "map:interior_null_before_L", "null:p0_null_p1_not_same_frame",
           "centre:one_joint", "centre:centre_frame_zero_while_p1_present"]
          + _rot("general", "general")),
    # the ABI limit with one person: survivors in every chunk, the last frame among them
    _case("t4_w2048", "t4", 2048, 4, 1, 2050, [[1, 2048]],
          [("keep", [(6, 2001, 37), 2048], 0)],
          ["scan:WM_at_limit_M1", "scan:compact_straddles_256", "map:compact",
           "map:wrap_many", "table:start_gt0", "centre:one_joint"]
          + _rot("general", "general")),
    # the ABI limit with two: person 0 keeps 40 frames with holes, person 1 is compacted
    # from every chunk, the last frame included
    _case("t4_w1024m2", "t4", 1024, 4, 2, 1024, [[0, 1024]],
          [("keep", [(0, 11), (14, 30), (33, 40)], 0), ("keep", [(3, 1024, 29), 1023], 1)],
          ["scan:WM_at_limit_M2", "scan:compact_straddles_256", "map:compact",
           "map:wrap_many", "map:interior_null_before_L", "null:p0_null_p1_not_same_frame",
           "centre:one_joint", "centre:centre_frame_zero_while_p1_present"]
          + _rot("general", "general")),
]
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


# --------------------------------------------------------------------------------------
# the branches a window reaches
# --------------------------------------------------------------------------------------
def clamped_rows(case):
    """The table as the kernel reads it: rows cut to the sequence and to W."""
    rows = []
    for s, r in case["table"]:
        s = min(max(int(s), 0), case["T"])
        rows.append((s, min(max(int(r), 0), min(case["W"], case["T"] - s))))
    return rows


def nonnull_flags(raw):
    """(M, W) bool: raw frame t of person m has a value that is not 0."""
    return np.transpose((raw != 0).any(axis=(0, 2)))


def _kind(v, e):
    """The branch of the rotation that turns v onto axis e, and its angle."""
    if np.abs(v).sum() < 1e-6:
        return "identity_l1", 0.0
    angle = po.align_angle(v, e)
    x, y, z = (float(c) for c in v)
    axis = (abs(y) + abs(x)) if e == 2 else (abs(z) + abs(y))
    if axis < 1e-6:
        return ("identity_axis_parallel" if v[e] > 0 else "identity_axis_antiparallel"), angle
    if abs(angle) < 1e-6:
        return "identity_theta", angle
    return "general", angle


def rotation_kinds(raw, skeleton, fp64=False, stages=7):
    """((z kind, z angle), (x kind, x angle)) of one zero-padded window, as
    ``po.normalize_window`` finds them under the stage mask (which decides whether the
    bones come from the padded and from the centred frame 0)."""
    p = po.normalize_window(raw.astype(np.float64 if fp64 else np.float32), skeleton,
                            stages & 3)
    zb, zt = skeleton["zaxis"]
    xr, xl = skeleton["xaxis"]
    vz = p[:, 0, zt, 0] - p[:, 0, zb, 0]
    p = po._rotate(p, po.align_matrix(vz, 2))
    return _kind(vz, 2), _kind(p[:, 0, xr, 0] - p[:, 0, xl, 0], 0)


def _window_tags(raw, nr, skeleton, first):
    C, W, V, M = raw.shape
    out = set()
    nn = nonnull_flags(raw)
    src = np.stack([po.source_map(f) for f in nn])
    for m in range(M):
        f = nn[m]
        idx = np.flatnonzero(f)
        if len(idx) == 0:
            out.add("map:absent")
            continue
        compact = not f[0]
        L = len(idx) if compact else int(idx[-1]) + 1
        if L == W:
            out.add("map:plain_full")
        elif W <= 2 * L:
            out.add("map:wrap_once")
        elif W >= 3 * L:
            out.add("map:wrap_many")
        if L == 1:
            out.add("map:L1")
        if compact:
            out.add("map:compact")
            if not first:
                out.add("table:compact_in_nonfirst_window")
            if len(idx) == 1:
                out.add("map:compact_count1")
            if idx[0] == 1 and idx[-1] == len(idx):
                out.add("map:compact_only_first_null")
            if idx[0] < 256 <= idx[-1]:
                out.add("scan:compact_straddles_256")
        elif not f[:L].all():
            out.add("map:interior_null_before_L")
        if idx[0] >= 256:
            out.add("scan:survivors_only_in_chunk1")
        if W > 192 and all(f[b - 1] != f[b] for b in (64, 128, 192)):
            out.add("scan:survivor_on_each_wave_boundary")
        real = raw[:, :nr, :, m]
        only_last_z = real[2, :, -1] != 0
        others = real.copy()
        others[2, :, -1] = 0
        if (only_last_z & ~others.any(axis=(0, 2))).any():
            out.add("null:nonnull_by_last_z_only")
        if (~f[:nr] & np.signbit(real).any(axis=(0, 2))).any():
            out.add("null:negzero_frame_is_null")
    if M >= 2:
        if (~nn[0, :nr] & nn[1, :nr]).any():
            out.add("null:p0_null_p1_not_same_frame")
        if not nn[0].any() and nn[1:].any():
            out.add("null:p0_absent_p1_present")
        if ((src[0] < 0) & (src[1:] >= 0).any(axis=0)).any():
            out.add("centre:centre_frame_zero_while_p1_present")
    padded = po.normalize_window(raw, skeleton, 1)
    absent = (padded[0] + padded[1]) + padded[2] == 0
    if (absent & (padded != 0).any(axis=0)).any():
        out.add("centre:joint_absent_by_cancellation")
    if raw.any():
        for a, (kind, _), joints in zip("zx", rotation_kinds(raw, skeleton),
                                        (skeleton["zaxis"], skeleton["xaxis"])):
            out.add(f"rot_{a}:{kind}")
            if absent[0, list(joints), 0].any():
                out.add(f"rot_{a}:axis_joint_absent_frame0")
    return out


def tags(case):
    """The set of branches of ``window_normalize_kernel`` the case reaches."""
    W, M = case["W"], case["M"]
    skeleton = SKELETONS[case["skel"]]
    out = {"centre:one_joint" if len(skeleton["center"]) == 1 else "centre:two_joint"}
    if W <= 256:
        out.add("scan:one_chunk")
    for w, mm, tag in ((256, M, "W256"), (257, M, "W257"), (300, 2, "two_chunks_M2"),
                       (2048, 1, "WM_at_limit_M1"), (1024, 2, "WM_at_limit_M2")):
        if (W, M) == (w, mm):
            out.add(f"scan:{tag}")
    seq = build(case["name"])
    rows = clamped_rows(case)
    for i, ((s, r), raw) in enumerate(zip(rows, po.cut_windows(seq, rows, W))):
        if s > 0:
            out.add("table:start_gt0")
        if r == 0:
            out.add("table:nr0")
        elif r < W:
            out.add("table:tail_window")
        out |= _window_tags(raw, r, skeleton, i == 0)
    return out


ROTATING = (4, 5, 6, 7)   # the stage masks that rotate


def windows_kinds(case, fp64=False, stages=7):
    """Per non-empty window, ((z kind, angle), (x kind, angle))."""
    return _kinds_of(case, build(case["name"]), fp64, stages)


def _kinds_of(case, seq, fp64, stages):
    skeleton = SKELETONS[case["skel"]]
    return [rotation_kinds(raw, skeleton, fp64, stages)
            for raw in po.cut_windows(seq, clamped_rows(case), case["W"]) if raw.any()]


def all_identity(case, stages=7):
    """Every rotation of the case is the identity under the stage mask: the output is then
    exact."""
    return all(k != "general" for win in windows_kinds(case, False, stages) for k, _ in win)


def _conditioned(case, seq):
    """Under every rotating stage mask, a general rotation has its angle in
    [0.2, pi - 0.2], and where any is general the float64 oracle takes the float32 one's
    branch for every rotation (the error-bar form compares the two)."""
    for stages in ROTATING:
        k32, k64 = _kinds_of(case, seq, False, stages), _kinds_of(case, seq, True, stages)
        flat = [(a, b) for w32, w64 in zip(k32, k64) for a, b in zip(w32, w64)]
        if all(kind != "general" for (kind, _), _ in flat):
            continue
        for (kind, angle), (kind64, _) in flat:
            if kind64 != kind or (kind == "general" and not 0.2 <= angle <= math.pi - 0.2):
                return False
    return True


@functools.lru_cache(maxsize=None)
def _build(name):
    case = BY_NAME[name]
    seed0 = 5003 + 97 * CASE_NAMES.index(name)
    for seed in range(seed0, seed0 + 3000, 3):
        seq = sequence(seed, case["T"], case["V"], case["M"])
        for e in case["edits"]:
            apply_edit(seq, e)
        if _conditioned(case, seq):
            seq.setflags(write=False)
            return seq
    raise AssertionError(f"{name}: no seed gives well-conditioned rotations")


def build(name):
    """The (3, T, V, M) float32 sequence of a case (read-only; shared between callers)."""
    return _build(name)


# --------------------------------------------------------------------------------------
# window_aggregate
# --------------------------------------------------------------------------------------
def _agg_rows(F):
    """Frames covered 0, 1 and 5 deep; a zero-length row, duplicate rows, rows out of table
    order, a row ending exactly at F and one running past it."""
    q = F // 4
    return [(2 * q, q), (q, 2 * q), (q, 2 * q), (F // 3, 0), (2 * q - 3, 10),
            (q + 1, 2 * q - 1), (F - 5, 5), (3, 1), (F - 2, 9)]


def _agg_case(name, F, rows, scores=None):
    return dict(name=name, total_frames=F, scores=scores,
                table=np.array(rows, dtype=np.int32).reshape(-1, 2))


AGG_CASES = [_agg_case(f"F{F}", F, _agg_rows(F)) for F in (255, 256, 257, 600)] + [
    _agg_case("F1", 1, [(0, 1), (0, 1), (0, 0), (0, 5)]),
    _agg_case("empty_table", 9, []),
    # ((1e16 + 1) - 1e16) + 1 = 1 in table order; 2 or 0 in any other
    _agg_case("table_order", 7, [(1, 5)] * 4, (1e16, 1.0, -1e16, 1.0)),
]


def agg_scores(case):
    """float64 (n_windows): the case's own scores, or formula values in (0, 1)."""
    if case["scores"] is not None:
        return np.array(case["scores"], dtype=np.float64)
    import formula
    return 0.5 + formula.hash_uniform(len(case["table"]), 9100 + case["total_frames"])


def agg_depths(case):
    cnt = np.zeros(case["total_frames"], dtype=np.int64)
    for s, r in case["table"]:
        cnt[s:s + r] += 1
    return cnt


# --------------------------------------------------------------------------------------
# sgcn_modalities
# --------------------------------------------------------------------------------------
def synthetic_parents(V):
    """A root that is its own parent (bone exactly 0) and parents V - 1 - v: larger than
    the child in the lower half."""
    par = np.array([V - 1 - v for v in range(V)], dtype=np.int32)
    par[0] = 0
    return par


# (N, C, T, V, M), parent table ("ntu" / "mp": the product's; "syn": synthetic_parents),
# data_bn on the plane layout as well
MOD_CASES = [
    ((1, 3, 1, 25, 2), "ntu", True),       # T = 1: both motions all zero
    ((2, 3, 5, 33, 1), "mp", False),
    ((1, 3, 7, 25, 2), "ntu", True),
    ((1, 2, 4, 8, 2), "syn", True),        # C != 3
    ((1, 5, 3, 4, 2), "syn", True),
    ((2, 2, 4, 8, 2), "syn", False),       # 256 elements: one full block
    ((1, 1, 1, 257, 1), "syn", False),     # 257: a second block of one thread
]


def mod_inputs(shape):
    """joint (N, C, T, V, M) and the data_bn scale / shift (4, M*V*C) of a case."""
    import formula
    N, C, T, V, M = shape
    seed = 300 + 7 * T + V + 1000 * C + M
    joint = formula.tensor(shape, seed, 1.0).numpy()
    scale = formula.tensor((4, M * V * C), seed + 1, 0.2, 1.0).numpy()
    shift = formula.tensor((4, M * V * C), seed + 2, 0.5).numpy()
    return joint, scale, shift


def to_planes(x):
    """(N, C, T, V, M) -> the model's (N*M, C, T, V)."""
    N, C, T, V, M = x.shape
    return np.ascontiguousarray(x.transpose(0, 4, 1, 2, 3)).reshape(N * M, C, T, V)


def data_bn_feature(shape):
    """The data_bn feature m*V*C + v*C + c of every element of the plane layout."""
    N, C, T, V, M = shape
    m, c, v = np.arange(M)[:, None, None, None], np.arange(C)[None, :, None, None], \
        np.arange(V)[None, None, None, :]
    f = np.broadcast_to((m * V + v) * C + c, (M, C, T, V))
    return np.ascontiguousarray(np.broadcast_to(f, (N,) + f.shape)).reshape(N * M, C, T, V)
