"""bench.py with TWO ranks on the one GPU of the test box: the multi-rank code path the driver launches on an 8-GPU
node (rank 0 builds and broadcasts the scene, every rank computes, SVF rows are gathered, times reduced over the ranks)
including everything only ranks > 0 execute.  RCCL refuses two ranks on one device, so the collectives run on gloo
(HZ_DIST_BACKEND; CUDA tensors are staged through host memory by horayzon_amd.dist) -- the bench code is the same."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(port, *args):
    env = dict(os.environ, HZ_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-cpu-baseline", *args]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])          # the JSON line is the last line of stdout


def test_config3_weak_replica_mode_with_two_ranks():
    d = _run(29621, "--tile", "601", "--azim", "72", "--steps", "2", "--warmup", "1", "--scaling", "weak")
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    cells = 569 * 569
    assert d["config"]["cells_per_step"] == cells
    # whole-job aggregate: both ranks' cells over the slowest rank's time
    assert abs(d["value"] - 2 * 2 * cells / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    assert d["config"]["scene_bcast_s"] > 0 and d["config"]["load_imbalance_max_over_mean"] >= 1.0
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["kernel_ms_per_launch"] > 0


def _plain(tmp_path, name, *args, gpus=1, backend="gloo"):
    """`python bench.py --gpus N ...` exactly as the driver types it: no torchrun, no rendezvous variables."""
    dump = str(tmp_path / (name + ".npy"))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["HZ_DIST_BACKEND"] = backend
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--tile", "601", "--azim", "72",
           "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-e2e", "--dump-svf-rows", "all", "--dump-path", dump, *args]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    return p, dump


def test_plain_bench_gpus_2_starts_two_ranks_and_shards_the_tile(tmp_path):
    """`python bench.py --gpus 2` (no torchrun) must itself start 2 ranks, run the STRONG-scaling row
    shard of the headline tile through dist.sharded_rows and gather the same SVF a single rank computes."""
    np = pytest.importorskip("numpy")
    dump_c5 = str(tmp_path / "c5_two.npy")
    p, dump2 = _plain(tmp_path, "two", "--full", "--c5-tile", "801", "--dump-c5-path", dump_c5, gpus=2)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 2 and d["value"] > 0
    # the N > 1 line also carries BASELINE config 5 run over the same ranks (extras.c5); `value` stays the c3 shard
    e5 = d["extras"]["c5"]
    assert e5["n_gpus"] == 2 and e5["cells_per_s"] > 0 and e5["scene_bcast_s"] > 0 and e5["job_s_incl_bcast"] >= e5["job_s"] > 0
    assert len(e5["slabs"]) == 2 and e5["slabs"][0][0] == 0 and e5["slabs"][0][1] == e5["slabs"][1][0] and e5["slabs"][1][1] == 769
    assert e5["load_imbalance_max_over_mean"] >= 1.0 and 1.0 <= e5["load_imbalance_predicted"] < 1.01 and e5["gathered_svf_finite"] is True
    assert "14401" not in e5["workload"] and "801x801" in e5["workload"]
    # ... whose gathered SVF is the SVF one rank computes for that mosaic
    env5 = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29628")
    dump_c5_one = str(tmp_path / "c5_one.npy")
    q5 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c5", "--tile", "801", "--azim", "72",
                         "--dump-svf-rows", "all", "--dump-path", dump_c5_one], cwd=ROOT, env=env5, capture_output=True, text=True, timeout=600)
    assert q5.returncode == 0, q5.stderr[-3000:]
    a5, b5 = np.load(dump_c5), np.load(dump_c5_one)
    assert a5.shape == (769, 769) and np.isfinite(a5).all() and np.array_equal(a5, b5)
    c = d["config"]
    sl = c["slabs"]
    assert len(sl) == 2 and sl[0][0] == 0 and sl[0][1] == sl[1][0] and sl[1][1] == 569 and 0 < sl[0][1] < 569   # disjoint, covering
    cells = 569 * 569
    assert c["cells_per_step"] == cells and abs(d["value"] - cells / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert c["gathered_svf_finite"] is True and len(c["t_ranks_s"]) == 2
    assert c["job_s_incl_bcast"] >= d["ms_per_step"] * 1e-3 and c["scene_bcast"] == "blob" and c["scene_bcast_bytes"] == c["scene_bytes"]
    assert d["roofline"]["kernel_ms_per_launch"] > 0
    # the sharded line carries the one-GPU emulation of its own partition next to what it measured
    sp = c["scaling_prediction"]
    assert "error" not in sp, sp
    assert len(sp["slab_ms_one_gpu"]) == 2 and sp["whole_tile_ms_one_gpu"] > 0
    assert 0.2 < c["predicted_efficiency"] <= 1.25 and c["predicted_efficiency"] == sp["predicted_efficiency"]
    assert sp["measured_efficiency_same_run"] > 0
    # one rank through the same sharded code path (HZ_FORCE_DIST) and the plain N = 1 line: the same SVF, bit for bit
    env1 = dict(os.environ, HZ_FORCE_DIST="1", HZ_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29626")
    dump1 = str(tmp_path / "one.npy")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--tile", "601", "--azim", "72", "--steps", "1", "--warmup", "0",
           "--no-cpu-baseline", "--no-e2e", "--no-count", "--no-peaks", "--dump-svf-rows", "all", "--dump-path", dump1]
    q = subprocess.run(cmd, cwd=ROOT, env=env1, capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, q.stderr[-3000:]
    d1 = json.loads(q.stdout.strip().splitlines()[-1])
    assert d1["n_gpus"] == 1 and d1["scaling"] == "strong" and d1["config"]["slabs"] == [[0, 569]]
    a, b = np.load(dump2), np.load(dump1)
    assert a.shape == (569, 569) and np.isfinite(a).all() and np.array_equal(a, b)
    # ... and the plain N = 1 line (one launch over the whole tile, no process group)
    r, dump0 = _plain(tmp_path, "plain", "--full", "--no-count", "--no-peaks", "--no-c5-extra", gpus=1)
    assert r.returncode == 0, r.stderr[-3000:]
    d0 = json.loads(r.stdout.strip().splitlines()[-1])
    assert d0["n_gpus"] == 1 and d0["scaling"] == "strong" and d0["config"]["cells_per_step"] == cells
    assert np.array_equal(a, np.load(dump0))
    # ... whose extras predict the N = 2 / 4 / 8 points of the strong-scaling curve from the slabs timed one by one
    pr = d0["extras"]["scaling_prediction"]
    assert "error" not in pr, pr
    for key, n_r in (("n2", 2), ("n4", 4), ("n8", 8)):
        assert len(pr[key]["slab_ms"]) == n_r and 0.1 < pr[key]["predicted_efficiency"] <= 1.25


def _gpus_visible():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def test_plain_bench_gpus_8_world_of_eight_on_one_gpu(tmp_path):
    """The world size the driver's scaling run ends with: `python bench.py --gpus 8` (eight ranks over gloo) -- eight
    disjoint slabs that cover the tile, every rank's time reported, the gathered SVF equal to the N = 1 SVF.  Runs where
    every rank has a GPU of its own: eight ranks on ONE device, with this process beside them, hold nine or more HIP
    contexts on it at once, more than a node shared with other jobs lets one device carry.  On one GPU,
    test_plain_bench_gpus_4_world_of_four_on_one_gpu runs these checks, and the config-5 job over the same ranks, for four."""
    have = _gpus_visible()
    if have < 8:
        pytest.skip("needs 8 GPUs (one per rank), found %d" % have)
    np = pytest.importorskip("numpy")
    p, dump8 = _plain(tmp_path, "eight", "--no-count", "--no-peaks", gpus=8)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    c = d["config"]
    sl = c["slabs"]
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and len(sl) == 8 and len(c["t_ranks_s"]) == 8
    assert sl[0][0] == 0 and sl[-1][1] == 569 and all(sl[i][1] == sl[i + 1][0] for i in range(7))
    assert all(71 <= b - a <= 72 for a, b in sl) and c["gathered_svf_finite"] is True
    assert c["cells_per_step"] == 569 * 569 and c["load_imbalance_max_over_mean"] >= 1.0
    r, dump1 = _plain(tmp_path, "one", "--no-count", "--no-peaks", "--no-extras", gpus=1)
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.load(dump8), np.load(dump1))


def test_plain_bench_gpus_4_world_of_four_on_one_gpu(tmp_path):
    """A world of four ranks on the one GPU of the test box (gloo): four disjoint slabs of 142 - 143 rows that cover the
    tile, every rank's time reported, the gathered SVF equal to the N = 1 SVF; then the config-5 job over the same four
    ranks (extras.c5, an 801^2 mosaic): four slabs that cover its 769 inner rows and a gathered SVF equal to one rank's."""
    np = pytest.importorskip("numpy")
    dump_c5 = str(tmp_path / "c5_four.npy")
    p, dump4 = _plain(tmp_path, "four", "--full", "--no-count", "--no-peaks", "--c5-tile", "801", "--dump-c5-path", dump_c5, gpus=4)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    c = d["config"]
    sl = c["slabs"]
    assert d["n_gpus"] == 4 and d["scaling"] == "strong" and len(sl) == 4 and len(c["t_ranks_s"]) == 4
    assert sl[0][0] == 0 and sl[-1][1] == 569 and all(sl[i][1] == sl[i + 1][0] for i in range(3))
    assert all(142 <= b - a <= 143 for a, b in sl) and c["gathered_svf_finite"] is True
    assert c["cells_per_step"] == 569 * 569 and c["load_imbalance_max_over_mean"] >= 1.0
    e5 = d["extras"]["c5"]
    s5 = e5["slabs"]
    assert e5["n_gpus"] == 4 and len(s5) == 4 and len(e5["t_ranks_s"]) == 4 and e5["gathered_svf_finite"] is True
    assert s5[0][0] == 0 and s5[-1][1] == 769 and all(s5[i][1] == s5[i + 1][0] for i in range(3))
    assert "801x801" in e5["workload"]
    r, dump1 = _plain(tmp_path, "one", "--no-count", "--no-peaks", "--no-extras", gpus=1)
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.load(dump4), np.load(dump1))
    env5 = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29629")
    dump_c5_one = str(tmp_path / "c5_one.npy")
    q5 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c5", "--tile", "801", "--azim", "72",
                         "--dump-svf-rows", "all", "--dump-path", dump_c5_one], cwd=ROOT, env=env5, capture_output=True, text=True, timeout=600)
    assert q5.returncode == 0, q5.stderr[-3000:]
    a5, b5 = np.load(dump_c5), np.load(dump_c5_one)
    assert a5.shape == (769, 769) and np.isfinite(a5).all() and np.array_equal(a5, b5)


def test_plain_bench_gpus_2_broadcasting_vertices_only(tmp_path):
    """--bcast verts: 12 V bytes on the links, every rank rebuilds the LBVH; same SVF as the blob broadcast."""
    np = pytest.importorskip("numpy")
    p, dump_v = _plain(tmp_path, "verts", "--bcast", "verts", "--no-count", "--no-peaks", gpus=2)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    c = d["config"]
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and c["scene_bcast"] == "verts"
    assert 12 * 601 * 601 <= c["scene_bcast_bytes"] < 12 * 601 * 601 + 256 and c["scene_bcast_bytes"] < c["scene_bytes"] / 4
    q, dump_b = _plain(tmp_path, "blob", "--no-count", "--no-peaks", gpus=2)
    assert q.returncode == 0, q.stderr[-3000:]
    assert np.array_equal(np.load(dump_v), np.load(dump_b))


def test_plain_bench_refuses_more_ranks_than_gpus():
    """RCCL needs one GPU per rank: `--gpus 9` on this box must fail loudly, not print an n_gpus = 1 line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HZ_DIST_BACKEND")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "9", "--tile", "601"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "GPU(s) visible" in (p.stderr + p.stdout) and "\"n_gpus\"" not in p.stdout


def test_config5_row_sharding_with_two_ranks():
    """Two ranks: only rank 0 synthesises the DEM, the blob is broadcast out of its own allocation, rank 1 derives its
    slab's inputs from the received vertices (slab-local, opts.inputs_are_slab), the slabs come from the sampled cost
    pre-pass (probe rows split over both ranks, joined by one all_reduce)."""
    d = _run(29622, "--workload", "c5", "--tile", "801", "--azim", "72", "--balance", "cost")
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    c = d["config"]
    slabs = c["slabs"]
    assert slabs[0][0] == 0 and slabs[0][1] == slabs[1][0] and slabs[1][1] == 769 and 300 < slabs[0][1] < 470
    assert c["gathered_svf_finite"] is True and len(c["t_ranks_s"]) == 2
    assert 1.0 <= c["load_imbalance_max_over_mean"] < 2.0
    assert "sampled cost" in c["parallelism"] and c["cost_prepass_probe_rows"] >= 16 and c["cost_prepass_s"] > 0
    assert 1.0 <= c["load_imbalance_predicted"] <= 1.02          # the split hits the cost target to within a row
    assert c["load_imbalance_predicted_if_balanced_by_cells"] >= c["load_imbalance_predicted"] - 1e-9
    assert c["scene_bcast_zero_copy"] is True and c["height_field"] == 1


def test_config5_single_rank_broadcast_is_free_and_emulated_partition():
    """One rank through the same code: the 'broadcast' out of the blob allocation costs nothing; --emulate-ranks times
    the slabs of a 4-rank partition one by one (the load balance a 4-GPU run would see)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29623")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c5", "--tile", "801", "--azim", "72"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1 and d["config"]["scene_bcast_s"] < 0.05 and d["config"]["gathered_svf_finite"] is True
    env["MASTER_PORT"] = "29624"
    p = subprocess.run(cmd + ["--emulate-ranks", "4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    e = json.loads(p.stdout.strip().splitlines()[-1])["config"]
    for kind in ("cost", "cells"):
        sl = e[kind]["slabs"]
        assert len(sl) == 4 and sl[0][0] == 0 and sl[-1][1] == 769 and all(sl[i][1] == sl[i + 1][0] for i in range(3))
        assert len(e[kind]["t_slab_s"]) == 4 and e[kind]["imbalance_measured"] >= 1.0
    assert e["cost"]["imbalance_predicted"] <= e["cells"]["imbalance_predicted"] + 1e-9


def test_config4_bench_line():
    """bench.py --workload c4 (small tile, 8 sun positions): the shadow line with its own roofline."""
    env = dict(os.environ)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c4", "--tile", "601", "--suns", "8", "--steps", "2",
           "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    cells = 569 * 569
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["unit"] == "cells/s" and "Terrain.shadow" in d["metric"]
    assert abs(d["value"] - 2 * 8 * cells / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["frac"] > 0.0 and r["kernel_ms_per_step"] > 0 and r["binding_resource"] == "valu_issue"
    assert 0.0 < r["frac_valu_counter_floor"] < r["frac_model_raw"] < 1.5
    assert r["nodes_per_ray"] > 1 and 0.0 < r["lane_utilisation_node_leaf_steps"] <= 1.0


def test_cost_balanced_slabs_pay_on_an_inhomogeneous_dem():
    """`--balance cost` on a DEM that is half rolling lowland (3 % of the relief), half high relief (--plain-fraction 0.5).  The two
    slabs of an emulated 2-rank partition are timed one after the other on the one GPU: split by cell count, one slab
    takes far longer than the other; split by the sampled cost pre-pass (probe rows bisected where neighbouring samples
    differ strongly, dist.estimate_row_cost) the two slabs take about the same."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29627")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c5", "--tile", "3073", "--azim", "120",
           "--plain-fraction", "0.5", "--emulate-ranks", "2", "--cost-samples", "48"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    e = json.loads(p.stdout.strip().splitlines()[-1])["config"]
    print(json.dumps({k: e[k] for k in ("cost", "cells")}))
    # Structural asserts only (timing thresholds on 0.23 s slabs do not belong in the gating suite): the cost
    # pre-pass moves the boundary towards the high relief, the predicted imbalance of the cost split is not worse than that of
    # the count split, every slab ran and the results were gathered.  The MEASURED imbalances are evidence, not a gate: they
    # are written to gpurun_out/balance_measured.json (copied to profiles/ by hand when a round quotes them).
    assert e["cost"]["slabs"][0][1] > e["cells"]["slabs"][0][1]          # the lowland's slab is longer
    assert e["cost"]["imbalance_predicted"] <= e["cells"]["imbalance_predicted"] + 1e-9
    assert e["cells"]["imbalance_predicted"] > 1.03                      # the cost model sees the inhomogeneity (deterministic)
    for kind in ("cost", "cells"):
        assert len(e[kind]["t_slab_s"]) == 2 and min(e[kind]["t_slab_s"]) > 0 and e[kind]["imbalance_measured"] >= 1.0
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "balance_measured.json"), "w") as fh:
        json.dump({k: e[k] for k in ("cost", "cells")}, fh, indent=1)
