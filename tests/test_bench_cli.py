"""bench.py's command line: a plain run prints the headline line only (every secondary section is behind --full), and
--dump-outputs writes the last timed step's outputs in a fixed, comparable form."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("roofline", "bf16_forward", "ddp_train", "ddp_train_bf16", "ddp_samples_per_s", "ddp_model", "cpu_baseline",
                  "forward_grad_enabled_eval_ms", "reference_loop_step_ms", "rollout_7x24h_vs_reference")
DUMP_LIMIT_BYTES = 64 * 2**20


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_full_is_off_by_default_and_steps_are_taken_as_given(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--steps", "3", "--full", "--dump-outputs", "d")
    assert (a.steps, a.full, a.dump_outputs) == (3, True, "d")
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_is_a_fixed_float32_sample_under_the_size_limit(tmp_path):
    g = torch.Generator().manual_seed(0)
    up = torch.randn((1, 5, 13, 721, 1440), generator=g)
    sfc = torch.randn((1, 4, 721, 1440), generator=g)
    for d in ("a", "b"):
        bench.dump_outputs((up, sfc), str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["output_sample.npy", "output_surface.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= DUMP_LIMIT_BYTES
    for f in files:      # same outputs in, same bytes out
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    s, o = np.load(tmp_path / "a" / "output_sample.npy"), np.load(tmp_path / "a" / "output_surface.npy")
    assert s.dtype == np.float32 and o.dtype == np.float32
    assert o.shape == (1, 4, 721, 1440) and np.array_equal(o, sfc.numpy())
    idx = np.sort(np.random.default_rng(0).choice(up.numel(), size=bench.DUMP_SAMPLE, replace=False))
    assert s.shape == (bench.DUMP_SAMPLE,) and np.array_equal(s, up.reshape(-1).numpy()[idx])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_its_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert all(k in d for k in CONTRACT_KEYS), d
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY_KEYS if k in d], sorted(d)
    s, o = np.load(tmp_path / "output_sample.npy"), np.load(tmp_path / "output_surface.npy")
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,) and np.isfinite(s).all()
    assert o.dtype == np.float32 and o.shape == (1, 4, 721, 1440) and np.isfinite(o).all()
    assert s.nbytes + o.nbytes <= DUMP_LIMIT_BYTES
