"""bench.py's command line without a GPU: it must refuse loudly (no CPU fallback, no fabricated line)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("gpus", ["1", "2"])
def test_bench_needs_a_gpu(gpus):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: covered by tests/test_gpu_bench_ranks.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", gpus], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "needs an MI355X" in (p.stderr + p.stdout) and '"metric"' not in p.stdout


def test_plain_run_times_its_steps_only(monkeypatch):
    """A plain run does what its headline figure needs: every untimed piece that takes runs of its own is off unless --full
    asks for it, and under --full the --no-* options still drop single pieces."""
    import bench
    extra = ("no_count", "no_peaks", "no_extras", "no_e2e", "no_c5_extra", "no_cpu_baseline")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and all(getattr(a, k) for k in extra) and (a.steps, a.warmup) == (3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert a.full and not any(getattr(a, k) for k in extra) and (a.steps, a.warmup) == (None, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-c5-extra"])
    a = bench.parse()
    assert a.no_c5_extra and not a.no_extras and not a.no_count


def test_dump_outputs_layout_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: the SVF of the last step's rows whole while it fits, the horizon at a fixed, seeded sample of cells
    (all azimuths), the (row, column) of every sampled cell; float32 / float64 only, the same files from run to run, and
    below 64 MB in all at the size of the c3 tile."""
    torch = pytest.importorskip("torch")
    import numpy as np
    import bench
    rows, in1, A, rb = 5, 7, 3, 4
    d_hori = torch.arange(rows * in1 * A, dtype=torch.float32).reshape(rows, in1, A)
    d_svf = torch.full((rb + rows + 2, in1), float("nan"))
    d_svf[rb:rb + rows] = torch.rand(rows, in1)
    shapes = bench.dump_step_outputs(str(tmp_path / "a"), d_hori, d_svf, rb, rb + rows)
    assert shapes == {"svf": [rows, in1], "hori_sample": [rows * in1, A], "hori_sample_cells": [rows * in1, 2]}
    load = lambda d, n: np.load(str(tmp_path / d / (n + ".npy")))
    assert load("a", "svf").dtype == np.float32 and np.array_equal(load("a", "svf"), d_svf[rb:rb + rows].numpy())
    cells, hori = load("a", "hori_sample_cells"), load("a", "hori_sample")
    assert cells.dtype == np.float64 and hori.dtype == np.float32
    r, c = cells[:, 0].astype(int) - rb, cells[:, 1].astype(int)
    assert np.array_equal(hori, d_hori.numpy()[r, c])
    # budgets below the data: seeded samples, identical in a second run
    monkeypatch.setattr(bench, "DUMP_SVF_BYTES", 20 * 5)
    monkeypatch.setattr(bench, "DUMP_HORI_BYTES", (4 * A + 16) * 6)
    for d in ("b", "c"):
        shapes = bench.dump_step_outputs(str(tmp_path / d), d_hori, d_svf, rb, rb + rows)
        assert shapes == {"svf_sample": [5], "svf_sample_cells": [5, 2], "hori_sample": [6, A], "hori_sample_cells": [6, 2]}
    for n in shapes:
        assert np.array_equal(load("b", n), load("c", n))
    cells = load("b", "svf_sample_cells").astype(int)
    assert len({tuple(x) for x in cells}) == 5 and (cells[:, 0] >= rb).all() and (cells[:, 0] < rb + rows).all()
    assert np.array_equal(load("b", "svf_sample"), d_svf.numpy()[cells[:, 0], cells[:, 1]])
    monkeypatch.undo()
    # the c3 tile (3569 x 3569 cells, 360 azimuths): whole SVF + sampled horizon; and the most a sampled SVF can take
    k = bench.DUMP_HORI_BYTES // (4 * 360 + 16)
    assert 3569 * 3569 * 4 <= bench.DUMP_SVF_BYTES and 3569 * 3569 * 4 + k * (4 * 360 + 16) < 64e6
    assert bench.DUMP_SVF_BYTES // 20 * 20 + bench.DUMP_HORI_BYTES < 64e6
