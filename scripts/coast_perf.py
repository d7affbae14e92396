"""Cost of ocean_masking.coastline_distance and coastline_buffer on a grid of the c3 tile's inner domain (3569^2 cells, about
half of them water, fractal coast), against the reference's own method on the same machine: SciPy's k-d tree with 16 workers,
the buffer in the reference's block form (block_size 11).

    python scripts/coast_perf.py [--n N] [--hurst H] [--thr METRES] [--repeats R] [--workers W] [--no-scipy] [--out FILE]

After one warm-up call, R timed calls of each of
  - distance_host / buffer_host:      NumPy arrays in, NumPy array out (the copies are part of the call)
  - distance_device / buffer_device:  torch tensors in HBM in and out
  - kdtree_distance / kdtree_buffer_blocks: SciPy (tree build included, as it is in the reference's functions)
For each: the median wall time with the least and the largest, and for the device passes the medians of the stats split (index
build, query, copies).  `identical`: the device result equals the k-d tree's bit for bit.  If SciPy is missing the comparison is
"not measured".  Prints one JSON line per pass (and writes them to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3569)
    ap.add_argument("--hurst", type=float, default=0.3)
    ap.add_argument("--thr", type=float, default=50000.0)
    ap.add_argument("--res", type=float, default=1.0 / 1200.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from horayzon_amd import ocean_masking as om
    from tests import coast_cases as cc
    g = cc.coast_grid(args.n, args.n, seed=3, hurst=args.hurst, res=args.res)
    x, y, z, land, pts, lat = g["x"], g["y"], g["z"], g["land"], g["pts"], g["lat"]
    water = ~land
    case = {"cells": int(land.size), "water_cells": int(water.sum()), "P": int(len(pts)), "dist_thr_m": args.thr,
            "res_deg": args.res}
    lines = []

    def report(name, walls, stats=None, identical=None, **extra):
        d = dict(case, **{"pass": name, "repeats": len(walls), "wall_ms_median": round(1e3 * float(np.median(walls)), 2),
                          "wall_ms_min": round(1e3 * min(walls), 2), "wall_ms_max": round(1e3 * max(walls), 2),
                          "identical": identical})
        if stats:
            for k, out in (("t_bvh_s", "build_ms"), ("t_kernel_s", "query_ms"), ("t_h2d_s", "h2d_ms"), ("t_d2h_s", "d2h_ms"),
                           ("t_total_s", "total_ms")):
                d[out + "_median"] = round(1e3 * float(np.median([s[k] for s in stats])), 3)
            d["scratch_bytes"] = stats[-1]["scratch_bytes"]
            d["num_cells"] = stats[-1]["num_cells"]
        d.update(extra)
        lines.append(d)
        print(json.dumps(d), flush=True)

    def timed(fn, sync=False):
        walls, stats, r = [], [], None
        for k in range(args.repeats + 1):
            t0 = time.perf_counter()
            r = fn()
            if sync:
                torch.cuda.synchronize()
            if k:                                               # the first call is the warm-up
                walls.append(time.perf_counter() - t0)
                stats.append(dict(om.last_stats))
        return r, walls, stats

    dev = [torch.from_numpy(a).cuda() for a in (x, y, z, land, pts)]
    torch.cuda.synchronize()
    d_host, w_dh, s_dh = timed(lambda: om.coastline_distance(x, y, z, land, pts))
    d_dev, w_dd, s_dd = timed(lambda: om.coastline_distance(*dev), sync=True)
    b_host, w_bh, s_bh = timed(lambda: om.coastline_buffer(x, y, z, land, pts, lat, args.thr, args.res, "sphere"))
    b_dev, w_bd, s_bd = timed(lambda: om.coastline_buffer(*dev, lat, args.thr, args.res, "sphere"), sync=True)
    same_dev = bool(np.array_equal(d_dev.cpu().numpy(), d_host, equal_nan=True) and np.array_equal(b_dev.cpu().numpy(), b_host))

    kd_d = kd_b = None
    walls_d = walls_b = None
    if not args.no_scipy:
        try:
            from scipy.spatial import KDTree
        except ImportError:
            KDTree = None
        if KDTree is not None:
            def kd_distance():
                tree = KDTree(pts)
                out = np.full(x.shape, np.nan)
                out[water] = tree.query(np.stack((x[water], y[water], z[water]), axis=1), k=1, workers=args.workers)[0]
                return out

            def kd_buffer(block_size=11):
                # the reference's coastline_buffer (ocean_masking.py:283-345): block centres, +- chord_max classes, the remainder
                chord = om.chord_max(lat, args.res, "sphere", block_size)
                tree = KDTree(pts)
                half = (block_size - 1) // 2
                sl = (slice(half, None, block_size), slice(half, None, block_size))
                shp = x[sl].shape
                d_c = tree.query(np.stack((x[sl].ravel(), y[sl].ravel(), z[sl].ravel()), axis=1), k=1,
                                 workers=args.workers)[0].reshape(shp)
                cls = np.full(shp, -1, np.int32)
                cls[d_c <= args.thr - chord] = 0
                cls[d_c > args.thr + chord] = 1
                out = np.full(x.shape, -1, np.int32)
                rep = np.repeat(np.repeat(cls, block_size, axis=0), block_size, axis=1)[:x.shape[0], :x.shape[1]]
                out[:rep.shape[0], :rep.shape[1]] = rep
                rem = out == -1
                out[rem] = tree.query(np.stack((x[rem], y[rem], z[rem]), axis=1), k=1, workers=args.workers)[0] > args.thr
                out[land] = 0
                return out.astype(bool)

            def cpu_timed(fn):
                walls, r = [], None
                for _ in range(max(1, min(args.repeats, 3))):
                    t0 = time.perf_counter()
                    r = fn()
                    walls.append(time.perf_counter() - t0)
                return r, walls
            kd_d, walls_d = cpu_timed(kd_distance)
            kd_b, walls_b = cpu_timed(kd_buffer)

    same_d = None if kd_d is None else bool(np.array_equal(d_host, kd_d, equal_nan=True))
    same_b = None if kd_b is None else bool(np.array_equal(b_host, kd_b))
    report("distance_host", w_dh, s_dh, same_d)
    report("distance_device", w_dd, s_dd, same_d if same_d is None else (same_d and same_dev))
    report("buffer_host", w_bh, s_bh, same_b, masked_cells=int(b_host.sum()))
    report("buffer_device", w_bd, s_bd, same_b if same_b is None else (same_b and same_dev), masked_cells=int(b_host.sum()))
    if kd_d is not None:
        report("kdtree_distance", walls_d, workers=args.workers)
        report("kdtree_buffer_blocks", walls_b, workers=args.workers, block_size=11)
        med = {d["pass"]: d["wall_ms_median"] for d in lines}
        summary = {"pass": "summary",
                   "kdtree_distance_over_distance_host": round(med["kdtree_distance"] / med["distance_host"], 2),
                   "kdtree_distance_over_distance_device": round(med["kdtree_distance"] / med["distance_device"], 2),
                   "kdtree_buffer_over_buffer_host": round(med["kdtree_buffer_blocks"] / med["buffer_host"], 2),
                   "kdtree_buffer_over_buffer_device": round(med["kdtree_buffer_blocks"] / med["buffer_device"], 2)}
    else:
        summary = {"pass": "summary", "kdtree": "not measured (SciPy is not installed or --no-scipy)"}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
