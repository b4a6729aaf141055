"""bench.py's command line on the host (no GPU): a plain run measures the headline only, `--full` restores the
supplementary measurements, and `--dump-outputs` writes float32 arrays that are the same from call to call."""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    return bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return _bench().parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_probe and a.no_sub and a.no_other and a.no_cpu_baseline


def test_full_restores_the_supplementary_measurements(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_probe or a.no_sub or a.no_other or a.no_cpu_baseline)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--dump-outputs", "d")
    assert a.no_cpu_baseline and not a.no_probe and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_arrays(tmp_path):
    bench = _bench()
    n = 100003
    flat = torch.arange(n, dtype=torch.float32)
    trainer = types.SimpleNamespace(store=types.SimpleNamespace(flat=flat, grad=-flat))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), trainer, torch.tensor(1.5))
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["grads_sample.npy", "loss.npy", "params_sample.npy"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss.npy"].tolist() == [1.5]
    p = a["params_sample.npy"]
    assert p.shape == (min(n, bench.DUMP_SAMPLE),) and (np.diff(p) >= 0).all() and 0 <= p[0] and p[-1] < n
    assert np.array_equal(a["grads_sample.npy"], -p)     # the same positions of both buffers
    for f, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f))
