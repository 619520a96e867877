"""Per-shape A/B of the eval-mode forward contractions, fp32 against bf16 operands (HIP events
around every C-ABI launch, keyed by launch shape): one MediaPipe member model's eval forward
at --batch windows, the two precisions alternated --rounds times in one process.
    python tools/bf16_shape_ab.py [--batch 256] [--rounds 3]
Prints, per (M, K, T, V, flags) contraction shape: launches per forward, fp32 and bf16
microseconds per launch, their ratio, and the bf16 launch's algorithmic TB/s."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "shift-gcn_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import shiftgcn  # noqa: E402
from shiftgcn import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
torch.manual_seed(1)
model = shiftgcn.Model(num_class=2, num_point=33, num_person=1,
                       graph="graph.mediapipe_pose.Graph").cuda().eval()
x = torch.randn(a.batch, 3, 300, 33, 1, generator=torch.Generator().manual_seed(0)).cuda()


def forward(precision):
    with torch.no_grad(), shiftgcn.eval_precision(precision):
        model(x)


for p in ("fp32", "bf16"):
    forward(p)
torch.cuda.synchronize()
tables = {}
for _ in range(a.rounds):
    for p in ("fp32", "bf16"):
        timer = ops.LaunchTimer(detail=True)
        ops.set_launch_timer(timer)
        forward(p)
        torch.cuda.synchronize()
        ops.set_launch_timer(None)
        for k, v in timer.summary().items():
            op, _, shape = k.partition(" ")
            if not op.startswith("pw_fwd"):
                continue
            # the two classes print the same shape fields except the fp32 one's mask / rotation
            # / accumulate flags, which the eval forward leaves at 0
            key = " ".join(f for f in shape.split()
                           if not f.startswith(("xrot", "mask", "acc")))
            d = tables.setdefault(key, {}).setdefault((p, op), [0, 0.0, 0.0])
            d[0] += v["launches"]
            d[1] += v["ms_total"]
            d[2] += v["bytes"]

print(f"{'n':>3} {'fp32 us':>9} {'bf16 us':>9} {'ratio':>6} {'bf16 TB/s':>9}  shape")
tot = {"fp32": 0.0, "bf16": 0.0}
for key, d in sorted(tables.items(), key=lambda kv: -sum(v[1] for v in kv[1].values())):
    f = d.get(("fp32", "pw_fwd"))
    b = d.get(("bf16", "pw_fwd_bf16")) or d.get(("bf16", "pw_fwd"))
    n = f[0] // a.rounds
    fu, bu = 1e3 * f[1] / f[0], 1e3 * b[1] / b[0]
    tot["fp32"] += f[1] / a.rounds
    tot["bf16"] += b[1] / a.rounds
    kind = "" if ("bf16", "pw_fwd_bf16") in d else "  (stays fp32)"
    tbs = b[2] / (b[1] * 1e-3) / 1e12
    print(f"{n:3d} {fu:9.1f} {bu:9.1f} {fu / bu:6.2f} {tbs:9.2f}  {key}{kind}")
print(f"contractions per forward: fp32 {tot['fp32']:.3f} ms, bf16 {tot['bf16']:.3f} ms")
