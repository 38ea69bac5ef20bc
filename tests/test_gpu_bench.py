"""bench.py on the GPU: a plain run (headline figure only) with --dump-outputs,
in this process (bench.main()), at 2 timed steps.  The dumped arrays are what
dense_fa_ left for the caller, from inputs that the seed fixes."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_timed_outputs(tmp_path, monkeypatch, capsys):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    import fa_hip
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FA_BENCH_CPU_STEP", "FA_BENCH_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    d = str(tmp_path / "dump")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                      "--settle-ms", "0", "--dump-outputs", d])
    assert bench.main() == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == bench.METRIC and out["unit"] == "TFLOP/s" and out["dtype"] == "bf16"
    assert out["higher_is_better"] is True and out["steps"] == 2 and out["warmup"] == 1
    flops = 4.0 * 64 * 4096 * 4096 * 64
    assert out["ms_per_step"] > 0
    assert abs(out["value"] - flops / (out["ms_per_step"] / 1e3) / 1e12) <= 1e-9 * out["value"]
    # a plain run measures nothing beside the headline figure
    assert out["full"] is False
    assert not {"cold", "clock", "clock_settle", "cfg2", "cfg3", "cfg4", "extra", "cpu_baseline"} & set(out)

    assert sorted(os.listdir(d)) == ["O.npy", "l.npy", "m.npy"]
    O, l, m = (np.load(os.path.join(d, n + ".npy")) for n in ("O", "l", "m"))
    N, dd, BH = bench.N_, bench.D_, bench.B_ * bench.H_
    assert O.shape == (bench.DUMP_ROWS, dd) and l.shape == m.shape == (N, 1, BH)
    assert O.dtype == l.dtype == m.dtype == np.float32
    assert O.nbytes + l.nbytes + m.nbytes <= 64 * 10 ** 6
    assert np.isfinite(O).all() and np.isfinite(l).all() and np.isfinite(m).all()

    # the same call on the same seeded inputs, outside the benchmark: identical bits
    gen = torch.Generator(device="cuda").manual_seed(1234)
    Q, K, V = (bench._randn_jl(fa_hip, (N, dd, BH), torch.bfloat16, gen) for _ in range(3))
    y, l2, m2 = fa_hip.dense_fa(Q, K, V)
    torch.cuda.synchronize()
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(N * BH, size=bench.DUMP_ROWS, replace=False))
    assert len(np.unique(rows)) == bench.DUMP_ROWS
    yn = y.float().cpu().numpy()
    assert np.array_equal(O, yn[rows % N, :, rows // N])
    assert np.array_equal(l, l2.cpu().numpy()) and np.array_equal(m, m2.cpu().numpy())
