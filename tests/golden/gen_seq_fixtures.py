"""Golden fixtures for the ``sgcn_window_normalize`` case table (``oracle/seq_cases.py``),
made by running the REFERENCE's own pre-normalisation on CPU: ``create_sliding_windows`` +
``pre_normalize`` (``inference_pipeline.py``) for the MediaPipe cases, and
``data_gen/preprocess.pre_normalization(data, zaxis, xaxis, center_joint)`` for the NTU
joints and the 4-joint test skeleton. Run only where ``/root/reference`` exists:

    python tests/golden/gen_seq_fixtures.py

The reference is imported exactly as ``gen_pipeline_fixtures.py`` imports it. Only results
are stored: ``<case>_ref32`` (float32 input) and, for the cases compared in error-bar form
(any rotation that is not the identity), ``<case>_d64``, the float32-rounded difference of
the float64-input result from it. The inputs are regenerated from the case's recipe.

Per case the generator asserts, with the reference's own ``_angle_between`` /
``angle_between`` and ``_rotation_matrix`` / ``rotation_matrix``, the branch that the case
table declares for each rotation (a ``general`` one has its angle in [0.2, pi - 0.2]), and
that "frame sums to zero" agrees with "frame is all zero" on every frame: a case with a
cancelling *joint* keeps its *frame* sums non-zero.

Output: ``tests/golden/seq_fixtures.npz``.
"""
from __future__ import annotations

import contextlib
import io
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_fixtures as gf  # noqa: E402
import gen_pipeline_fixtures as gp  # noqa: E402
import pipeline_oracle as po  # noqa: E402
from oracle import seq_cases as sc  # noqa: E402

REF = gf.REF


def main():
    gf._import_reference()
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda x, *a, **k: x
        sys.modules["tqdm"] = t
    for name in ("cv2", "mediapipe"):
        sys.modules.setdefault(name, types.ModuleType(name))
    for p in (REF, os.path.join(REF, "data_gen")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import inference_pipeline as ip  # noqa: E402
    import preprocess as ntu_pre  # noqa: E402

    def ref_normalize(wins, case):
        if case["skel"] == "mp":
            return ip.pre_normalize(wins.copy())
        joints = sc.SKELETONS[case["skel"]]
        with contextlib.redirect_stdout(io.StringIO()), \
                contextlib.redirect_stderr(io.StringIO()):
            return ntu_pre.pre_normalization(
                wins.copy(), zaxis=list(joints["zaxis"]), xaxis=list(joints["xaxis"]),
                center_joint=joints["center"][0])

    def reference_kind(v, e, angle, matrix):
        """The branch the reference's helpers take for bone v and unit axis e."""
        unit = [0, 0, 1] if e == 2 else [1, 0, 0]
        axis = np.cross(v, unit)
        a = angle(v, unit)
        identity = np.array_equal(matrix(axis, a), np.eye(3))
        if np.abs(v).sum() < 1e-6:
            kind = "identity_l1"
        elif np.abs(axis).sum() < 1e-6:
            kind = "identity_axis_parallel" if v[e] > 0 else "identity_axis_antiparallel"
        elif np.abs(a) < 1e-6:
            kind = "identity_theta"
        else:
            kind = "general"
        assert identity == (kind != "general"), (v, a)
        return kind, float(a), matrix(axis, a)

    def assert_reference_branches(stacked, case):
        """Both rotations of every non-empty window by the reference's own helpers, from
        the padded and centred frame 0, against the oracle's branch and the declared tags."""
        angle, matrix = ((ip._angle_between, ip._rotation_matrix) if case["skel"] == "mp" else
                         (ntu_pre.angle_between, ntu_pre.rotation_matrix))
        joints = sc.SKELETONS[case["skel"]]
        seen = set()
        for raw in stacked:
            if not raw.any():
                continue
            frame0 = po.normalize_window(raw, joints, 3)[:, 0, :, 0].T        # (V, 3)
            vz = frame0[joints["zaxis"][1]] - frame0[joints["zaxis"][0]]
            kz, az, mz = reference_kind(vz, 2, angle, matrix)
            present = frame0.sum(-1) != 0
            turned = frame0.copy()
            turned[present] = np.dot(frame0[present], mz.T)
            kx, ax, _ = reference_kind(
                turned[joints["xaxis"][0]] - turned[joints["xaxis"][1]], 0, angle, matrix)
            (oz, _), (ox, _) = sc.rotation_kinds(raw, joints)
            assert (kz, kx) == (oz, ox), (case["name"], kz, kx, oz, ox)
            for k, a in ((kz, az), (kx, ax)):
                assert k != "general" or 0.2 <= a <= math.pi - 0.2, (case["name"], k, a)
            seen |= {f"rot_z:{kz}", f"rot_x:{kx}"}
        declared = {t for t in case["tags"]
                    if t.startswith("rot_") and not t.endswith("axis_joint_absent_frame0")}
        assert seen == declared, (case["name"], seen, declared)

    out = {"case_names": np.array(sc.CASE_NAMES, dtype="U16")}
    for case in sc.CASES:
        name, W = case["name"], case["W"]
        seq = sc.build(name)
        rows = sc.clamped_rows(case)
        assert [list(r) for r in rows] == case["table"].tolist()
        stacked = po.cut_windows(seq, rows, W)
        if case["skel"] == "mp":
            # the reference's own cut of each row's frames
            for (s, r), raw in zip(rows, stacked):
                assert r > 0
                (win, s0, e0, r0), = ip.create_sliding_windows(seq[:, s:s + r], window_size=W)
                assert (s0, e0, r0) == (0, r, r) and np.array_equal(win, raw)
        gp.check_null_frames(stacked)
        assert_reference_branches(stacked, case)
        r32 = ref_normalize(stacked, case)
        r64 = ref_normalize(stacked.astype(np.float64), case)
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        out[f"{name}_ref32"] = r32
        if not sc.all_identity(case):
            out[f"{name}_d64"] = (r64 - r32.astype(np.float64)).astype(np.float32)
        print(name, case["table"].tolist(), "max|ref32 - ref64| =",
              float(np.abs(r32 - r64).max()))
    path = os.path.join(HERE, "seq_fixtures.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
