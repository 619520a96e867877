"""Evaluation on the device (csrc/evaluate.hip, shiftgcn/evaluate.py) against its closed
forms restated on the CPU in float64 (numpy / torch); the rank and prediction rules are the
numpy statements of tests/test_eval_host.py.

Bars:
* pred, rank, hit counts, confusion matrix: exact.
* fused scores: bit-equal to the numpy expression of ensemble.py:27 in the scores' type.
* loss_i: within 1 float32 ulp of the float64 reference rounded to float32. The reference is
  ``log1p(sum_{c != argmax} exp(r_c - m)) + (m - r_l)`` in numpy float64: the same quantity as
  torch's float64 cross-entropy (checked here at 1e-12), written without a cancelling term
  so that it is itself accurate where the loss is far below the spacing of logsumexp(r)
  (confident rows at +-1e4). The device's float64 exp / log1p are within a few float64 ulps,
  so after one rounding to float32 the two differ at a rounding boundary at most.
* batch mean: 1e-12 relative of the float64 mean of the reference losses.
* two runs: bit-identical.
* sgcn_ce_bwd / train.cross_entropy: dlogits within 1 float32 ulp of the float64 reference
  rounded to float32.
* train_step(loss_fn=train.cross_entropy) against the default step: the block bars of
  DESIGN.md §Parity bars (loss 2e-5 relative, parameter gradients 1e-4 of the tensor's
  maximum, both with the 2e-5 floor of tests/test_gpu_blocks.py).
Every output sits in front of a guard region (and behind ``row_offset`` untouched rows) that
must keep its sentinel.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

import formula
from test_eval_host import pred_rule, rank_rule

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 67
FSENT, ISENT = -777.25, -123456
CS = [2, 5, 60, 64, 65, 120, 130]
NS = [1, 3, 64, 65, 257]
ALPHA = (0.6, 0.6, 0.4, 0.4)


# ----------------------------------------------------------------------------------------
# data and the CPU rule
# ----------------------------------------------------------------------------------------
def make_scores(kind, n, C, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    if kind == "random":
        s = rng.standard_normal((n, C)).astype(dtype)
    elif kind == "big":       # exp overflows without the maximum shift
        s = rng.uniform(-1e4, 1e4, (n, C)).astype(dtype)
    else:                     # three distinct values: many ties
        s = np.array([-1.5, 0.0, 2.25], dtype=dtype)[rng.integers(0, 3, (n, C))]
    while kind != "ties":     # tie-free rows: redraw the few that repeat a value
        rep = [i for i, row in enumerate(s) if len(np.unique(row)) != C]
        if not rep:
            break
        s[rep] = (s[rep] + rng.standard_normal((len(rep), C)) * 0.5).astype(dtype)
    labels = rng.integers(0, C, n)
    if kind == "ties":        # the label at both ends of its tie group
        for i in range(n):
            same = np.flatnonzero(s[i] == s[i, labels[i]])
            if i % 3 == 0:
                labels[i] = same[0]
            elif i % 3 == 1:
                labels[i] = same[-1]
    return s, labels.astype(np.int64)


def cpu_rule(r, labels, topk):
    """float64 closed forms on the (n, C) rows ``r`` (the scores the metrics are taken of)."""
    n, C = r.shape
    r64 = r.astype(np.float64)
    pred = pred_rule(r)
    rank = rank_rule(r, labels)
    valid = (labels >= 0) & (labels < C)
    m = r64.max(axis=1)
    e = np.exp(r64 - m[:, None])
    e[np.arange(n), pred] = 0.0
    l1p = np.log1p(e.sum(axis=1))
    lc = np.where(valid, labels, 0)
    loss = np.where(valid, l1p + (m - r64[np.arange(n), lc]), np.nan)
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (labels[valid], pred[valid]), 1)
    hits = [int((rank[valid] < k).sum()) for k in topk]
    return dict(pred=pred, rank=rank, loss=loss, lse=m + l1p, confusion=conf, hits=hits,
                bad=int((~valid).sum()))


def ulp32_close(dev, ref):
    a, b = np.asarray(dev).astype(np.float32), np.asarray(ref).astype(np.float32)
    ok = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b))
    return bool(np.all(ok | (np.isnan(a) & np.isnan(b))))


def run_kernel(scores, labels, weights=None, topk=(), off=0):
    """One sgcn_score_metrics + sgcn_batch_loss on sentinel-filled buffers with guard regions;
    returns the written regions and asserts that nothing else changed."""
    from shiftgcn.evaluate import batch_loss, score_metrics
    st = torch.from_numpy(np.ascontiguousarray(scores)).to(DEV)
    lt = torch.from_numpy(labels).to(DEV)
    n, C = st.shape[-2:]
    rows, nk = off + n, len(topk)

    def fbuf(shape, dt):
        return torch.full(shape, FSENT, device=DEV, dtype=dt)

    def ibuf(count, zeros):
        b = torch.full((count + GUARD,), ISENT, device=DEV, dtype=torch.int32)
        b[:zeros] = 0
        return b
    fused = fbuf((rows + GUARD, C), st.dtype)
    loss, lse = fbuf((rows + GUARD,), torch.float64), fbuf((rows + GUARD,), torch.float64)
    bl = fbuf((3 + GUARD,), torch.float64)
    pred, rank = ibuf(rows, 0), ibuf(rows, 0)
    hits, conf, bad = ibuf(nk, nk), ibuf(C * C, C * C), ibuf(1, 1)
    score_metrics(st, lt, weights, topk, off, fused, loss, lse, pred, rank, hits,
                  conf[:C * C], bad[:1])
    batch_loss(loss, off, n, bl, 2)
    out = {k: v.cpu().numpy() for k, v in dict(fused=fused, loss=loss, lse=lse, pred=pred,
                                               rank=rank, hits=hits, confusion=conf, bad=bad,
                                               batch_loss=bl).items()}
    for name in ("fused", "loss", "lse"):
        assert np.all(out[name][:off] == FSENT) and np.all(out[name][rows:] == FSENT), name
        out[name] = out[name][off:rows]
    for name in ("pred", "rank"):
        assert np.all(out[name][:off] == ISENT) and np.all(out[name][rows:] == ISENT), name
        out[name] = out[name][off:rows]
    for name, cnt in (("hits", nk), ("confusion", C * C), ("bad", 1)):
        assert np.all(out[name][cnt:] == ISENT), name
        out[name] = out[name][:cnt]
    b = out["batch_loss"]
    assert np.all(b[:2] == FSENT) and np.all(b[3:] == FSENT)
    out["batch_loss"] = b[2]
    out["confusion"] = out["confusion"].reshape(C, C)
    return out


def check_against_rule(out, ref, n):
    assert np.array_equal(out["pred"], ref["pred"])
    assert np.array_equal(out["rank"], ref["rank"])
    assert list(out["hits"]) == ref["hits"]
    assert np.array_equal(out["confusion"], ref["confusion"])
    assert int(out["bad"][0]) == ref["bad"]
    assert ulp32_close(out["loss"], ref["loss"])
    assert np.allclose(out["lse"], ref["lse"], rtol=1e-14, atol=1e-14)
    if ref["bad"] == 0:
        mean = ref["loss"].mean()
        assert abs(out["batch_loss"] - mean) <= 1e-12 * abs(mean)


# ----------------------------------------------------------------------------------------
# sgcn_score_metrics / sgcn_batch_loss
# ----------------------------------------------------------------------------------------
def test_reference_is_torchs_float64_cross_entropy():
    for kind in ("random", "big", "ties"):
        s, y = make_scores(kind, 65, 60, 5)
        ref = cpu_rule(s, y, ())
        want = torch.nn.functional.cross_entropy(torch.from_numpy(s).double(),
                                                 torch.from_numpy(y), reduction="none").numpy()
        assert np.allclose(ref["loss"], want, rtol=1e-12, atol=1e-12), kind
        assert np.allclose(ref["lse"], torch.logsumexp(torch.from_numpy(s).double(), 1).numpy(),
                           rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("kind", ["random", "ties", "big"])
@pytest.mark.parametrize("C", CS)
def test_metrics_match_cpu_rule(C, kind):
    topk = (1, 5, C, C + 3)
    for j, n in enumerate(NS):
        s, y = make_scores(kind, n, C, 1000 * C + n)
        ref = cpu_rule(s, y, topk)
        for off in ((0, 11) if j % 2 else (5, 0)):
            out = run_kernel(s, y, None, topk, off)
            check_against_rule(out, ref, n)
            assert np.array_equal(out["fused"], s)       # S = 1: the scores as they are
        if kind == "random":
            d = make_scores(kind, n, C, 1000 * C + n, np.float64)[0]
            check_against_rule(run_kernel(d, y, None, topk, 3), cpu_rule(d, y, topk), n)


def test_two_runs_are_bit_identical():
    s, y = make_scores("random", 257, 130, 3)
    stack = np.stack([s, s[::-1], s * 2, s - 1]).astype(np.float32)
    for scores, w in ((s, None), (stack, ALPHA)):
        a = run_kernel(scores, y, w, (1, 5), 4)
        b = run_kernel(scores, y, w, (1, 5), 4)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("C,n", [(60, 257), (2, 65), (130, 64), (5, 3)])
def test_fusion_is_bit_equal_to_ensemble_py(C, n):
    rng = np.random.default_rng(C + n)
    for dtype in (np.float32, np.float64):
        r = [rng.standard_normal((n, C)).astype(dtype) * 7 for _ in range(4)]
        y = rng.integers(0, C, n).astype(np.int64)
        alpha = list(ALPHA)
        want = r[0] * alpha[0] + r[1] * alpha[1] + r[2] * alpha[2] + r[3] * alpha[3]
        assert want.dtype == dtype
        out = run_kernel(np.stack(r), y, alpha, (1, 5), 2)
        assert out["fused"].tobytes() == want.tobytes()
        check_against_rule(out, cpu_rule(want, y, (1, 5)), n)
        # ensemble.py's own loop (tie-free rows: numpy's default sort agrees)
        assert all(len(np.unique(row)) == C for row in want)
        right = sum(int(np.argmax(want[i]) == y[i]) for i in range(n))
        right5 = sum(int(y[i] in want[i].argsort()[-5:]) for i in range(n))
        assert list(out["hits"]) == [right, right5]


def test_fuse_scores_api():
    from shiftgcn import fuse_scores
    rng = np.random.default_rng(8)
    n, C = 65, 60
    names = [f"S{i:03d}" for i in range(n)]
    mats = [rng.standard_normal((n, C)).astype(np.float32) for _ in range(4)]
    y = rng.integers(0, C, n)
    dicts = [dict(zip(names, m)) for m in mats[:2]] + mats[2:]
    res = fuse_scores(dicts, (names, [int(v) for v in y]))
    a = list(ALPHA)
    want = mats[0] * a[0] + mats[1] * a[1] + mats[2] * a[2] + mats[3] * a[3]
    assert res["scores"].tobytes() == want.tobytes()
    ref = cpu_rule(want, y.astype(np.int64), (1, 5))
    assert res["topk"] == {1: ref["hits"][0] / n, 5: ref["hits"][1] / n}
    assert np.array_equal(res["pred"], ref["pred"]) and np.array_equal(res["rank"], ref["rank"])
    assert np.array_equal(res["confusion"], ref["confusion"])
    assert abs(res["mean_loss"] - ref["loss"].mean()) <= 1e-12 * ref["loss"].mean()
    with pytest.raises(ValueError):
        fuse_scores(mats[:1], y, weights=(1.0,))


@pytest.mark.parametrize("C,n", [(5, 65), (64, 3), (130, 257)])
def test_bad_labels(C, n):
    from shiftgcn import ScoreMetrics
    s, y = make_scores("random", n, C, 77 + C)
    y[0], y[n - 1] = -1, C
    if n > 2:
        y[1] = 2 ** 40
    ref = cpu_rule(s, y, (1, C + 3))
    assert ref["bad"] == min(n, 3) and ref["confusion"].sum() == n - ref["bad"]
    out = run_kernel(s, y, None, (1, C + 3), 6)
    check_against_rule(out, ref, n)
    bad = (y < 0) | (y >= C)
    assert np.all(np.isnan(out["loss"][bad])) and not np.any(np.isnan(out["loss"][~bad]))
    assert np.all(out["rank"][bad] == C)
    assert np.isnan(out["batch_loss"])
    # the same run without the bad rows leaves the same confusion matrix
    good = run_kernel(s[~bad], y[~bad], None, (1, C + 3), 0)
    assert np.array_equal(good["confusion"], out["confusion"])
    assert list(good["hits"]) == list(out["hits"])
    sm = ScoreMetrics(C, topk=(1, 5), capacity=n, device=DEV)
    sm.update(torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV))
    with pytest.raises(ValueError, match="labels outside"):
        sm.result()


def test_score_metrics_object_over_batches():
    from shiftgcn import ScoreMetrics
    C, n = 65, 257
    s, y = make_scores("ties", n, C, 21)
    ref = cpu_rule(s, y, (1, 5, C + 3))
    st, yt = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    for cap in (n, None):
        sm = ScoreMetrics(C, topk=(1, 5, C + 3), capacity=cap, device=DEV)
        cuts = [0, 64, 65, 130, 257]
        for a, b in zip(cuts[:-1], cuts[1:]):
            sm.update(st[a:b], yt[a:b])
        res = sm.result()
        means = [ref["loss"][a:b].mean() for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.allclose(res["batch_loss"], means, rtol=1e-12, atol=0)
        assert abs(res["mean_loss"] - np.mean(means)) <= 1e-12 * np.mean(means)
        assert res["topk"] == {k: h / n for k, h in zip((1, 5, C + 3), ref["hits"])}
        assert np.array_equal(res["confusion"], ref["confusion"])
        sup = ref["confusion"].sum(1)
        want = np.diag(ref["confusion"])[sup > 0] / sup[sup > 0]
        assert np.array_equal(res["per_class_accuracy"][sup > 0], want)
        if cap:
            assert np.array_equal(res["pred"], ref["pred"])
            assert np.array_equal(res["rank"], ref["rank"])
            assert res["scores"].tobytes() == s.tobytes()
        else:
            assert res["pred"] is None and res["scores"] is None


# ----------------------------------------------------------------------------------------
# sgcn_ce_bwd and train.cross_entropy
# ----------------------------------------------------------------------------------------
def ce_bwd_reference(s, y, g):
    r = torch.from_numpy(s).double()
    p = torch.softmax(r, dim=1).numpy()
    n, C = s.shape
    valid = (y >= 0) & (y < C)
    p[np.arange(n)[valid], y[valid]] -= 1.0
    p[~valid] = 0.0
    return p * float(g) / n


@pytest.mark.parametrize("C", [2, 5, 60, 65, 130])
def test_ce_bwd_and_cross_entropy(C):
    from shiftgcn import train
    from shiftgcn.evaluate import ce_bwd, score_metrics
    for n, scale in ((1, 1.0), (3, 3.0), (65, 1.0), (257, 3.0)):
        s, y = make_scores("random", n, C, 31 * C + n)
        s = (s * np.float32(scale)).astype(np.float32)
        if n > 2:
            y[1] = C        # a bad row: zeros
        st, yt = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
        g = torch.tensor(0.37, device=DEV)
        _, lse = score_metrics(st, yt)
        d = ce_bwd(st, lse, yt, g).cpu().numpy()
        assert ulp32_close(d, ce_bwd_reference(s, y, np.float32(0.37)))
        if n > 2:
            assert np.all(d[1] == 0)
            y[1] = 0
            yt = torch.from_numpy(y).to(DEV)
        # the autograd Function: float32 mean loss, backward through sgcn_ce_bwd
        x = st.clone().requires_grad_(True)
        loss = train.cross_entropy(x, yt)
        assert loss.dtype == torch.float32 and loss.shape == ()
        loss.backward()
        ref = cpu_rule(s, y, ())
        assert ulp32_close(loss.item(), ref["loss"].mean())
        assert ulp32_close(x.grad.cpu().numpy(), ce_bwd_reference(s, y, 1.0))


def _train_setup():
    import shiftgcn
    m = shiftgcn.Model(num_class=10, num_point=25, num_person=2, graph="graph.ntu_rgb_d.Graph")
    formula.fill_state(m, seed=9)
    m = m.to(DEV).train()
    x = formula.tensor((2, 3, 32, 25, 2), 77, 1.0).to(DEV)
    y = torch.tensor([1, 7], device=DEV)
    return m, x, y


def _rel_close(a, b, tol, what, floor=2e-5):
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= tol * scale + floor, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def test_train_step_with_native_loss_matches_default():
    from shiftgcn import train
    m, x, y = _train_setup()
    m2 = copy.deepcopy(m)
    opt, opt2 = train.build_optimizer(m, base_lr=0.1), train.build_optimizer(m2, base_lr=0.1)
    la = train.train_step(m, opt, x, y)
    lb = train.train_step(m2, opt2, x, y, loss_fn=train.cross_entropy)
    _rel_close(lb.detach().cpu(), la.detach().cpu(), 2e-5, "loss")
    for (name, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        if p.requires_grad:
            _rel_close(q.grad.cpu(), p.grad.cpu(), 1e-4, f"grad {name}")


def test_graph_captured_step_replays_to_the_same_loss(monkeypatch):
    from shiftgcn import ops, train
    # capturing a training step switches the eval caches off for the process: keep it here
    monkeypatch.setattr(ops, "_CAPTURED_WRITES", False)
    m, x, y = _train_setup()
    m2 = copy.deepcopy(m)
    opt, opt2 = train.build_optimizer(m, base_lr=0.1), train.build_optimizer(m2, base_lr=0.1)
    ce = train.cross_entropy
    for _ in range(4):
        eager = train.train_step(m, opt, x, y, loss_fn=ce)
    for _ in range(2):
        train.train_step(m2, opt2, x, y, loss_fn=ce)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        train.train_step(m2, opt2, x, y, loss_fn=ce)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = train.train_step(m2, opt2, x, y, loss_fn=ce)
    g.replay()                                   # the fourth step of m2
    torch.cuda.synchronize()
    assert torch.equal(captured.detach(), eager.detach())
    for (name, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), name


# ----------------------------------------------------------------------------------------
# evaluate()
# ----------------------------------------------------------------------------------------
def _write_dataset(tmp_path, shape, num_class, seed):
    rng = np.random.default_rng(seed)
    data = rng.standard_normal(shape).astype(np.float32)
    labels = [int(v) for v in rng.integers(0, num_class, shape[0])]
    names = [f"clip{i:03d}.skeleton" for i in range(shape[0])]
    np.save(tmp_path / "data.npy", data)
    with open(tmp_path / "label.pkl", "wb") as f:
        pickle.dump((names, labels), f)
    from shiftgcn.feeder import Feeder
    return Feeder(str(tmp_path / "data.npy"), str(tmp_path / "label.pkl")), data, names, labels


def test_evaluate_model(tmp_path):
    import shiftgcn
    from shiftgcn.evaluate import evaluate_async
    from shiftgcn.feeder import DeviceBatchLoader
    C, bs = 5, 3
    fd, data, names, labels = _write_dataset(tmp_path, (7, 3, 16, 25, 2), C, 1)
    m = shiftgcn.Model(num_class=C, num_point=25, num_person=2, graph="graph.ntu_rgb_d.Graph")
    formula.fill_state(m, seed=5)
    m = m.to(DEV).eval()
    xs = torch.from_numpy(data).to(DEV)
    with torch.no_grad():
        want = torch.cat([m(xs[i:i + bs]) for i in range(0, 7, bs)]).cpu().numpy()
    y = np.asarray(labels, dtype=np.int64)

    # nothing in the loop reads the device: only result() does
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metrics = evaluate_async(m, DeviceBatchLoader(fd, bs, shuffle=False), topk=(1, 5, 2))
        with pytest.raises(RuntimeError, match="synchroniz"):
            metrics.result()                  # the run's one read-back is what the mode sees
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res0 = metrics.result()
    assert res0["scores"].tobytes() == want.tobytes()

    files = [str(tmp_path / f) for f in ("wrong.txt", "result.txt", "score.pkl")]
    res = shiftgcn.evaluate(m, DeviceBatchLoader(fd, bs, shuffle=False), topk=(1, 5, 2),
                            wrong_file=files[0], result_file=files[1], score_file=files[2])
    assert res["scores"].dtype == np.float32 and res["scores"].tobytes() == want.tobytes()
    assert res["n"] == 7
    assert all(len(np.unique(row)) == C for row in want)
    assert res["topk"] == {k: fd.top_k(want, k) for k in (1, 5, 2)}
    w64 = torch.from_numpy(want).double()
    means = [float(torch.nn.functional.cross_entropy(w64[i:i + bs], torch.from_numpy(y[i:i + bs])))
             for i in range(0, 7, bs)]
    assert abs(res["mean_loss"] - np.mean(means)) <= 1e-6 * abs(np.mean(means))
    ref = cpu_rule(want, y, (1, 5, 2))
    assert np.array_equal(res["pred"], ref["pred"]) and np.array_equal(res["rank"], ref["rank"])
    assert np.array_equal(res["confusion"], ref["confusion"])
    # the files of main.py:488-492 and :506-515 for these scores
    pred = want.argmax(1)
    assert open(files[1]).read() == "".join(f"{p},{t}\n" for p, t in zip(pred, y))
    assert open(files[0]).read() == "".join(f"{i},{p},{t}\n" for i, (p, t) in
                                            enumerate(zip(pred, y)) if p != t)
    with open(files[2], "rb") as f:
        sd = pickle.load(f)
    assert list(sd) == names
    assert all(sd[nm].tobytes() == want[i].tobytes() for i, nm in enumerate(names))

    with pytest.raises(ValueError, match="shuffle"):
        shiftgcn.evaluate(m, DeviceBatchLoader(fd, bs, shuffle=True))
    fd.label[2] = C
    with pytest.raises(ValueError, match="labels outside"):
        shiftgcn.evaluate(m, DeviceBatchLoader(fd, bs, shuffle=False))


def test_evaluate_ensemble(tmp_path):
    import shiftgcn
    from shiftgcn import ensemble as ens
    from shiftgcn.feeder import DeviceBatchLoader
    C, n, bs = 2, 5, 2
    fd, data, names, labels = _write_dataset(tmp_path, (n, 3, 16, 33, 1), C, 2)
    models = []
    for k in range(4):
        mm = shiftgcn.Model(num_class=C, num_point=33, num_person=1,
                            graph="graph.mediapipe_pose.Graph")
        formula.fill_state(mm, seed=701 + 13 * k)
        models.append(mm.to(DEV).eval())
    e = ens.Ensemble(models).to(DEV)
    xs = torch.from_numpy(data).to(DEV)
    want = torch.cat([e(xs[i:i + bs])[1] for i in range(0, n, bs)]).cpu().numpy()
    assert want.dtype == np.float64
    res = shiftgcn.evaluate(e, DeviceBatchLoader(fd, bs, shuffle=False), topk=(1, 2))
    # full batches through the graph, the last one eagerly: the same bits either way
    assert res["scores"].dtype == np.float64 and res["scores"].tobytes() == want.tobytes()
    y = np.asarray(labels, dtype=np.int64)
    ref = cpu_rule(want, y, (1, 2))
    assert np.array_equal(res["pred"], ref["pred"]) and np.array_equal(res["rank"], ref["rank"])
    assert res["topk"] == {1: ref["hits"][0] / n, 2: ref["hits"][1] / n}
    assert np.array_equal(res["confusion"], ref["confusion"])
    means = [ref["loss"][i:i + bs].mean() for i in range(0, n, bs)]
    assert abs(res["mean_loss"] - np.mean(means)) <= 1e-12 * abs(np.mean(means))
