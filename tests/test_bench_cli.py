"""bench.py's options, output dump and rank handling on the CPU (nothing here touches a GPU;
``tests/test_gpu_bench_outputs.py`` runs a plain benchmark on one).

Config 5 (``main.py:294-299``, ``device: [0,1,2,3]`` in
``config/nturgbd-cross-subject/train_joint.yaml:35``) is measured by ``bench.py --gpus N``:
without a launcher it starts the N ranks itself (``launch_command``, a child
``torch.distributed.run``); under a launcher the launcher's WORLD_SIZE must equal ``--gpus``.
The end-to-end two-rank line (``world_size`` / ``backend`` in ``config``) is
``tests/test_gpu_dist.py::test_bench_two_ranks_same_device``.
"""
import os
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_check_world_rules():
    assert bench.check_world(1, {}) == 1
    assert bench.check_world(8, {}) is None                 # start the 8 ranks first
    assert bench.check_world(4, {"WORLD_SIZE": "4"}) == 4
    with pytest.raises(SystemExit) as e:
        bench.check_world(8, {"WORLD_SIZE": "1"})
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        bench.check_world(1, {"WORLD_SIZE": "2"})


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_times_the_steps_only(monkeypatch):
    """Without ``--full`` the legs after the timed region (roofline steps, CPU baseline) are
    off whatever their own switches say; ``--full`` runs them, each with its own off switch."""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.roofline, a.cpu_baseline) == (7, 3, False, 0, 0)
    assert a.dump_outputs is None
    a = _parse(monkeypatch, "--roofline", "1", "--cpu-baseline", "1")
    assert (a.roofline, a.cpu_baseline) == (0, 0)
    a = _parse(monkeypatch, "--full")
    assert a.full and (a.roofline, a.cpu_baseline) == (1, 1)
    a = _parse(monkeypatch, "--full", "--cpu-baseline", "0", "--dump-outputs", "d")
    assert (a.roofline, a.cpu_baseline, a.dump_outputs) == (1, 0, "d")


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--steps", "-1"), ("--warmup", "-1")])
def test_step_counts_are_validated(monkeypatch, argv):
    with pytest.raises(SystemExit) as e:
        _parse(monkeypatch, *argv)
    assert e.value.code == 2


def test_dump_outputs_writes_float_arrays(tmp_path):
    import numpy as np
    import torch
    named = [("loss", torch.tensor([1.5])),
             ("param.l1.w", torch.arange(6, dtype=torch.float32).reshape(2, 3)),
             ("scores", torch.tensor([0.25, 0.75], dtype=torch.float64)),
             ("buffer.n", torch.tensor(2 ** 40 + 1))]
    out = tmp_path / "o" / "p"                    # (created as needed)
    bench.dump_outputs(str(out), named)
    assert sorted(p.name for p in out.iterdir()) == sorted(n + ".npy" for n, _ in named)
    for name, t in named:
        a = np.load(out / (name + ".npy"), allow_pickle=False)
        assert a.dtype == (np.float32 if t.dtype == torch.float32 else np.float64), name
        assert a.shape == tuple(t.shape) and np.array_equal(a, t.numpy()), name


def test_dump_outputs_samples_above_the_size_limit(tmp_path, monkeypatch):
    """Above the limit every array keeps the same fraction of its elements: a sorted sample
    of the flattened array, the same elements in every run."""
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    named = [("a", torch.arange(4000, dtype=torch.float32).reshape(40, 100)),
             ("b", torch.arange(1000, dtype=torch.float64)), ("c", torch.tensor([3.0]))]
    got = []
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), named)
        got.append({n: np.load(tmp_path / d / (n + ".npy")) for n, _ in named})
    assert sum(a.nbytes for a in got[0].values()) <= 4096
    for n, t in named:
        a = got[0][n]
        assert np.array_equal(a, got[1][n]) and a.ndim == 1, n
        assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < max(t.numel(), 4), n
    # (values are the flat indices here) a real sample, not a prefix; the same fraction each
    assert got[0]["a"][-1] > 2000 and got[0]["c"].size == 1
    assert abs(got[0]["a"].size / 4000 - got[0]["b"].size / 1000) < 0.01


def test_launch_command_runs_this_bench_under_torchrun():
    cmd = bench.launch_command(["--gpus", "8", "--steps", "5"], 8, 29999)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29999" in cmd
    i = cmd.index(os.path.join(REPO, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "5"]


@pytest.mark.parametrize("env_ws, gpus", [("2", "1"), ("1", "8"), ("4", "2")])
def test_world_size_mismatch_exits_nonzero(env_ws, gpus):
    env = dict(os.environ, WORLD_SIZE=env_ws, RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", gpus,
                        "--steps", "1", "--warmup", "0"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=REPO)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "WORLD_SIZE" in r.stderr and not r.stdout.strip()


def test_more_ranks_than_visible_gpus_exits_nonzero():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")}
    env["HIP_VISIBLE_DEVICES"] = ""   # (no GPU in this container anyway)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "8",
                        "--steps", "1"], env=env, capture_output=True, text=True,
                       timeout=300, cwd=REPO)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "GPUs are visible" in r.stderr
