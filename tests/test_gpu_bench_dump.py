"""bench.py --dump-outputs on the GPU: what the last timed step computed lands in DIR/<name>.npy, the same files from run to
run with the same arguments, and --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HZ_FORCE_DIST")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tile", "601", "--azim", "72", "--warmup", "1",
           "--no-cpu-baseline", "--no-e2e", "--no-count", "--no-peaks", "--no-extras", "--dump-outputs", str(out), *args]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_of_the_last_timed_step(tmp_path, hip):
    whole = str(tmp_path / "svf_all.npy")
    d = _bench(tmp_path / "a", "--steps", "3", "--dump-svf-rows", "all", "--dump-path", whole)
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert abs(d["value"] - 569 * 569 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    a = _load(str(tmp_path / "a"))
    assert d["config"]["dump_outputs"] == {k: list(v.shape) for k, v in a.items()}
    assert set(a) == {"svf", "hori_sample", "hori_sample_cells"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) < 64e6
    assert np.array_equal(a["svf"], np.load(whole)) and np.isfinite(a["svf"]).all()
    assert a["hori_sample"].shape[1] == 72 and np.isfinite(a["hori_sample"]).all()
    # what a caller of the public API receives for the same tile and parameters (bench.py's defaults: dist_search 50 km,
    # guess_constant, hori_acc 0.25 deg, SVF over the planar tilt)
    from horayzon_amd import synth
    g = synth.fractal_tile(n=601, offset=16)
    kw = {k: g[k] for k in ("vert_grid", "dem_dim_0", "dem_dim_1", "vec_norm", "vec_north", "offset_0", "offset_1")}
    vec_tilt, _ = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], 16)
    hori, _, svf = hip.horizon.horizon_gridded(**kw, dist_search=50.0, azim_num=72, svf_vec_tilt=vec_tilt)
    cr = a["hori_sample_cells"].astype(int)
    assert np.array_equal(a["hori_sample"], hori[cr[:, 0], cr[:, 1]])
    assert np.array_equal(a["svf"], svf)
    # same arguments, same inputs: the same outputs
    assert _bench(tmp_path / "b", "--steps", "1")["steps"] == 1
    b = _load(str(tmp_path / "b"))
    assert set(b) == set(a) and all(np.array_equal(a[k], b[k]) for k in a)
    # slab steps: the last of 2 timed steps (after 1 warm-up) covers the third slab of 200 rows, rows 400 .. 568
    s = _bench(tmp_path / "s", "--steps", "2", "--rows-per-step", "200")
    assert s["steps"] == 2
    c = _load(str(tmp_path / "s"))
    assert np.array_equal(c["svf"], a["svf"][400:569])
    rows = c["hori_sample_cells"][:, 0]
    assert (rows >= 400).all() and (rows < 569).all()
    # the horizon of a cell does not depend on the slab it was computed in
    key = {tuple(x): i for i, x in enumerate(a["hori_sample_cells"].astype(int).tolist())}
    both = [(key[tuple(x)], j) for j, x in enumerate(c["hori_sample_cells"].astype(int).tolist()) if tuple(x) in key]
    assert len(both) > 100
    for i, j in both:
        assert np.array_equal(a["hori_sample"][i], c["hori_sample"][j])
