"""The eval-mode "bf16" inference precision (shiftgcn.eval_precision, Ensemble(precision=))
on units, whole models and the ensemble, and its plumbing.

Numerics. E is the distance of the float64 oracle with the device's rounding points
(tests/bf16_emulation.py) from the plain float64 oracle (oracle/model_oracle.py), D the
device bf16 path's distance from the same float64 oracle. Condition: rms(D) <= 2 * rms(E)
over tensors of at least 100 values — the project's bar style ("no further from fp64 than 2 x
the reference is"): after a few layers the device's and the emulation's roundings are
independent realisations of the same noise, so the ratio is about 1. E is computed at run
time on the CPU; rms(E), rms(D) and the fp32 path's own distance are printed for each case.
The ensemble's three scores and six logits are too few for a statistical bar: printed only.

Plumbing: which launches the setting changes (by ops.LaunchTimer classes), that the default
path is bit-identical and makes none of the new launches, that a forward which can be
back-propagated stays fp32, the constructor argument, the environment default (fresh child
process), and hipGraph replay of the bf16 ensemble.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import formula
from bf16_emulation import emulate_bf16
from conftest import GOLDEN, PKG_ROOT, REPO
from oracle import model_oracle as mo
from oracle import torch_shift as ts

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def float64_shift(monkeypatch):
    """The oracle's temporal shift in the dtype of its input (the numpy one is float32)."""
    monkeypatch.setattr(mo.Shift, "function", ts.TorchShiftFunction)


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _report(what, d_bf16, d_fp32, e):
    """Print the three distances; assert rms(D) <= 2 rms(E) on >= 100 values."""
    rd, r32, re = _rms(d_bf16), _rms(d_fp32), _rms(e)
    print(f"{what}: n {e.numel()} rms(E) {re:.3e} rms(D) {rd:.3e} ratio {rd / re:.3f} "
          f"fp32 path {r32:.3e}")
    assert e.numel() >= 100 and re > 0
    assert rd <= 2 * re, (what, rd, re)
    return rd, re


def _oracle64(ref, emulate):
    m = copy.deepcopy(ref).double().eval()
    return emulate_bf16(m) if emulate else m


def _launches(fn):
    """{launch class: count} of the C-ABI launches fn() makes, and its result."""
    from shiftgcn import ops
    timer = ops.LaunchTimer()
    ops.set_launch_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_launch_timer(None)
    torch.cuda.synchronize()
    counts = {}
    for rec in timer.records:
        counts[rec[0]] = counts.get(rec[0], 0) + 1
    return counts, out


def _pw(counts):
    return counts.get("pw_fwd", 0), counts.get("pw_fwd_bf16", 0)


# --------------------------------------------------------------------------------------
# single units
# --------------------------------------------------------------------------------------
UNITS = [
    # (C_in, C_out, stride, residual, V, K >= 32 contractions, K < 32 contractions)
    (64, 64, 1, True, 25, 2, 0),       # identity residual
    (64, 128, 2, True, 25, 4, 0),      # gcn down conv + conv residual
    (128, 256, 2, True, 33, 4, 0),
    (3, 64, 1, False, 25, 1, 2),       # l1: gcn Linear and down conv stay fp32
]


@pytest.mark.parametrize("cin,cout,stride,residual,V,n_bf16,n_fp32", UNITS,
                         ids=lambda v: str(int(v)))
def test_unit(cin, cout, stride, residual, V, n_bf16, n_fp32):
    import shiftgcn
    ref = mo.TCN_GCN_unit(cin, cout, None, stride=stride, residual=residual, num_point=V)
    formula.fill_state(ref, seed=11 + cin + cout + V)            # non-trivial running stats
    ref.eval()
    ours = shiftgcn.TCN_GCN_unit(cin, cout, None, stride=stride, residual=residual,
                                 num_point=V).to(DEV)
    ours.load_state_dict(ref.state_dict())
    ours.eval()
    x = formula.tensor((2, cin, 8, V), 5 + cin, 1.0)
    with torch.no_grad():
        y64 = _oracle64(ref, False)(x.double())
        yE = _oracle64(ref, True)(x.double())
        xd = x.to(DEV)
        c32, y32 = _launches(lambda: ours(xd))
        with shiftgcn.eval_precision("bf16"):
            cbf, ybf = _launches(lambda: ours(xd))
    assert c32.get("pw_fwd_bf16", 0) == 0 and c32["pw_fwd"] == n_bf16 + n_fp32
    assert cbf.get("pw_fwd_bf16", 0) == n_bf16 and cbf.get("pw_fwd", 0) == n_fp32
    _report(f"unit {cin}->{cout} s{stride} V{V}", ybf.cpu().double() - y64,
            y32.cpu().double() - y64, yE - y64)


# --------------------------------------------------------------------------------------
# whole models
# --------------------------------------------------------------------------------------
MODELS = {"ntu": (60, 25, 2, "graph.ntu_rgb_d.Graph"),
          "mp": (2, 33, 1, "graph.mediapipe_pose.Graph")}
N_BF16, N_FP32 = 23, 2     # contractions of one forward with K >= 32 / l1's two with K = 3


def _fc_input(model, run):
    """(what run() returns, the fc input it saw)."""
    seen = []
    h = model.fc.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach()))
    try:
        out = run()
    finally:
        h.remove()
    return out, seen[-1]


@pytest.mark.parametrize("name", list(MODELS))
def test_model(name):
    """bs = 2 at the shapes of tests/golden/gen_fixtures.py (T = 300): the fc input (2 x 256)
    and, for NTU, the 2 x 60 logits; the launch classes of one forward."""
    import shiftgcn
    num_class, V, M, graph = MODELS[name]
    k = sum(map(ord, name))
    ref = mo.Model(num_class=num_class, num_point=V, num_person=M)
    formula.fill_state(ref, seed=97 + k)
    ref.eval()
    ours = shiftgcn.Model(num_class=num_class, num_point=V, num_person=M, graph=graph).to(DEV)
    ours.load_state_dict(ref.state_dict())
    ours.eval()
    x = formula.tensor((2, 3, 300, V, M), 41 + k, 1.0)
    with torch.no_grad():
        m64, mE = _oracle64(ref, False), _oracle64(ref, True)
        l64, f64 = _fc_input(m64, lambda: m64(x.double()))
        lE, fE = _fc_input(mE, lambda: mE(x.double()))
        xd = x.to(DEV)
        (c32, l32), f32 = _fc_input(ours, lambda: _launches(lambda: ours(xd)))
        with shiftgcn.eval_precision("bf16"):
            (cbf, lbf), fbf = _fc_input(ours, lambda: _launches(lambda: ours(xd)))
        (c32b, l32b), _ = _fc_input(ours, lambda: _launches(lambda: ours(xd)))
    assert c32.get("pw_fwd_bf16", 0) == 0 and c32["pw_fwd"] == N_BF16 + N_FP32
    assert cbf["pw_fwd_bf16"] == N_BF16 and cbf["pw_fwd"] == N_FP32
    # the default path after the context manager was used: the launches and bits of before
    # (the first forward also computes the cached eval constants: compare the contractions)
    assert _pw(c32b) == _pw(c32) and torch.equal(l32b, l32)
    assert not torch.equal(lbf, l32)
    _report(f"model {name} fc input", fbf.cpu().double() - f64, f32.cpu().double() - f64,
            fE - f64)
    if name == "ntu":
        _report("model ntu logits", lbf.cpu().double() - l64, l32.cpu().double() - l64,
                lE - l64)


def test_differentiable_eval_forward_stays_fp32():
    """Grad enabled and parameters requiring grad: a backward may follow, so the "bf16"
    setting changes nothing (no bf16 launch, the fp32 bits)."""
    import shiftgcn
    ours = shiftgcn.TCN_GCN_unit(64, 128, None, stride=2, residual=True, num_point=25).to(DEV)
    formula.fill_state(ours, seed=3)
    ours.eval()
    assert all(p.requires_grad for p in ours.parameters() if p.dtype.is_floating_point)
    x = formula.tensor((2, 64, 8, 25), 9, 1.0).to(DEV)
    c0, y0 = _launches(lambda: ours(x))
    with shiftgcn.eval_precision("bf16"):
        c1, y1 = _launches(lambda: ours(x))
        with torch.no_grad():
            c2, y2 = _launches(lambda: ours(x))
    assert y1.requires_grad and _pw(c1) == _pw(c0) == (4, 0)
    assert torch.equal(y1, y0)
    assert c2["pw_fwd_bf16"] == 4 and not torch.equal(y2, y0)
    y1.sum().backward()                                   # and the backward runs
    assert ours.gcn1.Linear_weight.grad is not None


# --------------------------------------------------------------------------------------
# ensemble
# --------------------------------------------------------------------------------------
def _members():
    import shiftgcn
    models = []
    for k in range(4):
        m = shiftgcn.Model(num_class=2, num_point=33, num_person=1,
                           graph="graph.mediapipe_pose.Graph")
        formula.fill_state(m, seed=701 + 13 * k)
        models.append(m.to(DEV).eval())
    return models


def _ensemble(precision=None, **kw):
    from shiftgcn import ensemble as ens
    return ens.Ensemble(_members(), precision=precision, **kw).to(DEV)


def _streams64(joint, parent):
    """derive_modalities (inference_pipeline.py:284-309), float64 on the CPU."""
    bone = joint - joint[:, :, :, parent.long(), :]
    T = joint.shape[2]

    def motion(a):
        out = torch.zeros_like(a)
        out[:, :, :T - 1] = a[:, :, 1:] - a[:, :, :T - 1]
        return out

    return [joint, bone, motion(joint), motion(bone)]


def test_ensemble_fc_inputs_and_scores():
    """The three windows of tests/golden/ensemble_fixtures.npz: the four members' fc inputs
    (4 x 3 x 256 values) under the RMS condition; scores and logits printed."""
    fx = np.load(os.path.join(GOLDEN, "ensemble_fixtures.npz"), allow_pickle=False)
    wins = torch.from_numpy(fx["ens_windows"])
    e32, ebf = _ensemble("fp32"), _ensemble("bf16")
    assert e32.precision == "fp32" and ebf.precision == "bf16"

    def run(e):
        seen = []
        hooks = [m.fc.register_forward_pre_hook(lambda mod, a: seen.append(a[0].detach().cpu()))
                 for m in e.models]
        try:
            scores, logits = e(wins.to(DEV))
        finally:
            for h in hooks:
                h.remove()
        torch.cuda.synchronize()
        return scores.cpu(), logits.cpu(), torch.stack(seen).double()

    s32, l32, f32 = run(e32)
    sbf, lbf, fbf = run(ebf)
    f64, fE = [], []
    acc = torch.zeros(3, 2, dtype=torch.float64)
    with torch.no_grad():
        streams = _streams64(wins.double(), e32.parent.cpu())
        for k, (m, s) in enumerate(zip(e32.models, streams)):
            ref = mo.Model(num_class=2, num_point=33, num_person=1)
            ref.load_state_dict({n: v.cpu() for n, v in m.state_dict().items()})
            ref.eval()
            m64, mE = _oracle64(ref, False), _oracle64(ref, True)
            logit, f = _fc_input(m64, lambda: m64(s))
            f64.append(f)
            fE.append(_fc_input(mE, lambda: mE(s))[1])
            acc += float(np.float32(e32.weights[k])) * logit
    f64, fE = torch.stack(f64), torch.stack(fE)
    ex = torch.exp(acc - acc.max(dim=1, keepdim=True).values)
    s64 = ex[:, 1] / ex.sum(dim=1)
    _report("ensemble fc inputs", fbf - f64, f32 - f64, fE - f64)
    print("scores  fixture", fx["ens_scores"], "\n        float64", s64.numpy(),
          "\n        fp32   ", s32.numpy(), "\n        bf16   ", sbf.numpy())
    print("logits  float64", acc.numpy().ravel(), "\n        fp32   ", l32.numpy().ravel(),
          "\n        bf16   ", lbf.numpy().ravel())
    print(f"max |score bf16 - fp32| {float((sbf - s32).abs().max()):.3e}  "
          f"max |logit bf16 - fp32| {float((lbf - l32).abs().max()):.3e}")
    assert not torch.equal(lbf, l32)


def test_ensemble_precision_argument():
    from shiftgcn import ensemble as ens
    from shiftgcn import fused
    models = _members()
    with pytest.raises(ValueError):
        ens.Ensemble(models, precision="int8")
    assert ens.Ensemble(models).precision == fused.EVAL_PRECISION
    # the argument wins over an enclosing context, and the context is restored
    e = ens.Ensemble(models, precision="fp32").to(DEV)
    x = formula.tensor((2, 3, 48, 33, 1), 901, 1.0).to(DEV)
    with fused.eval_precision("bf16"):
        counts, _ = _launches(lambda: e(x))
        assert fused.current_eval_precision() == "bf16"
    assert counts.get("pw_fwd_bf16", 0) == 0
    counts, _ = _launches(lambda: ens.Ensemble(models, precision="bf16").to(DEV)(x))
    assert counts["pw_fwd_bf16"] == 4 * N_BF16 and counts["pw_fwd"] == 4 * N_FP32


def test_environment_default_in_a_fresh_process():
    code = (
        "import torch, formula, shiftgcn\n"
        "from shiftgcn import fused, ops, ensemble as ens\n"
        "assert fused.EVAL_PRECISION == 'bf16' == fused.current_eval_precision()\n"
        "u = shiftgcn.TCN_GCN_unit(64, 64, None, stride=1, residual=True, num_point=25).cuda()\n"
        "formula.fill_state(u, seed=3); u.eval()\n"
        "t = ops.LaunchTimer(); ops.set_launch_timer(t)\n"
        "with torch.no_grad(): u(formula.tensor((2, 64, 8, 25), 9, 1.0).cuda())\n"
        "ops.set_launch_timer(None); torch.cuda.synchronize()\n"
        "n = sum(r[0] == 'pw_fwd_bf16' for r in t.records)\n"
        "print('bf16 launches', n)\n")
    env = dict(os.environ, SGCN_EVAL_PRECISION="bf16",
               PYTHONPATH=os.pathsep.join([PKG_ROOT, REPO, GOLDEN]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert "bf16 launches 2" in r.stdout


def test_ensemble_graph_replay_equals_eager_bf16():
    from shiftgcn.ensemble import EnsembleGraph
    e = _ensemble("bf16")
    e32 = _ensemble("fp32")
    N, T = 6, 48
    x1 = formula.tensor((N, 3, T, 33, 1), 901, 1.0).to(DEV)
    x2 = formula.tensor((N, 3, T, 33, 1), 902, 1.0).to(DEV)
    g = EnsembleGraph(e, x1.shape, DEV)
    for x in (x1, x2, x1):
        s_eager, l_eager = e(x)
        s_g, l_g = g.run(x)
        torch.cuda.synchronize()
        assert torch.equal(s_g, s_eager) and torch.equal(l_g, l_eager)
    assert not torch.equal(l_eager, e32(x1)[1])           # and it is the bf16 result


def test_sequence_scorer_graph_equals_eager_bf16():
    """100 frames, window 64, stride 32: the graphed scorer's per-frame scores are the eager
    ones (both hold the bf16 launches)."""
    from shiftgcn import pipeline
    e = _ensemble("bf16")
    seq = formula.tensor((3, 100, 33, 1), 77, 1.0).numpy()
    graphed = pipeline.SequenceScorer(e, 64, 32, batch=2, graph=True)
    eager = pipeline.SequenceScorer(e, 64, 32, batch=2, graph=False)
    pf_g, sc_g, table = graphed.score(seq)
    pf_e, sc_e, _ = eager.score(seq)
    assert pf_g.shape == (100,) and len(table) == sc_g.shape[0] > 1
    assert torch.equal(pf_g, pf_e) and torch.equal(sc_g, sc_e)
    e32 = _ensemble("fp32")
    assert not torch.equal(pipeline.SequenceScorer(e32, 64, 32, batch=2, graph=False)
                           .score(seq)[1], sc_e)
