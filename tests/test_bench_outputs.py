"""bench.py's plain run and --dump-outputs.

* dump_outputs on a stand-in engine (CPU): every array a caller of engine.step() receives is
  written as float32 / float64 .npy; past the 64 MB budget an array is cut to a sample that
  is the same from call to call, and the files stay within the budget.
* A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` on the GPU: one JSON
  line with the headline fields and none of the --full ones, K really the number of timed
  steps, and the dumped logits / losses those of the line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench

FULL_ONLY = ("step_distribution", "roofline", "spmm_roofline", "gemm_roofline", "head_roofline",
             "kernels_ms_per_step", "sub_configs", "cpu_baseline", "dropin", "epoch_with_eval_ms")


class _Engine:
    def __init__(self, n):
        g = torch.Generator().manual_seed(1)
        self._logits = torch.rand(n, 12, generator=g).to(torch.bfloat16)
        self._w = torch.randn(7, 5, generator=g)

    def logits(self):
        return self._logits

    def losses(self):
        return [0.25, 0.5]

    def state_dict(self):
        return {"liner2.weight": self._w}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_array(tmp_path):
    eng = _Engine(100)
    bench.dump_outputs(eng, str(tmp_path / "o"))
    got = _load(tmp_path / "o")
    assert sorted(got) == ["logits", "loss", "param.liner2.weight"]
    assert got["logits"].dtype == np.float32 and got["param.liner2.weight"].dtype == np.float32
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [0.25, 0.5]
    assert np.array_equal(got["logits"], eng.logits().float().numpy())
    assert np.array_equal(got["param.liner2.weight"], eng._w.numpy())


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3000)  # logits alone: 100 x 12 x 4 = 4800 B
    eng = _Engine(100)
    bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 3000
    assert a["logits"].size == 250 and np.array_equal(a["logits"], b["logits"])
    assert np.isin(a["logits"], eng.logits().float().numpy()).all()
    assert np.array_equal(a["param.liner2.weight"], eng._w.numpy())  # within its share: whole


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    steps = 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "2", "--dump-outputs", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == 2 and out["n_gpus"] == 1
    assert out["unit"] == "edges/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    # value is edges per second over the timed steps (both rounded in the line)
    assert out["value"] == pytest.approx(out["config"]["edges_per_step"] / (out["ms_per_step"] / 1e3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in out]
    got = _load(tmp_path / "o")
    assert got["logits"].shape == (out["config"]["nodes"], 12) and got["logits"].dtype == np.float32
    assert np.isfinite(got["logits"]).all()
    assert got["loss"].tolist() == [out["loss"]["train"], out["loss"]["val"]]
    assert got["param.liner2.weight"].shape == (12, 100)
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
