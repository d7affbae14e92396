"""Cost of Terrain.sight_height on the c3 tile (synth.fractal_tile: 3601^2, offset 16) against Terrain.viewshed(facing=False)
-- the same ray, one per cell -- in the same process: per observer and, what the comparison is about, per ray.

    python scripts/sight_height_perf.py [--tile N] [--repeats R] [--out FILE] [--label TEXT]

Everything is device resident (observers and outputs are torch tensors in HBM; the height tables are NumPy, staged once per
call).  Observers are 2 - 10 m above DEM vertices on a regular lattice (scripts/viewshed_perf.py), one of them or 16.  After
one warm-up of every pass, the passes are run R times in alternation; per pass the median kernel time of last_stats (HIP
events around the launches), its range, and the wall time of a call that ends in a device synchronise.  Passes, each with 1
and 16 observers, each without and with max_dist = 5000:
  - viewshed:      viewshed(visible=..., facing=False, target_elev=0.05)
  - sight_129:     sight_height(height=...) with sight_heights(256.05, 2.0)   (129 entries)
  - sight_1025:    sight_height(height=...) with sight_heights(256.05, 0.25)  (1025 entries)
Prints one JSON line per pass -- ms per observer, rays, rays per cell in range, ns per ray -- then the ratios of the ns per ray
to the viewshed's of the same observers and range, and writes them to --out (profiles/sight/sight_perf.jsonl holds a run on an
MI355X).  --label goes into every line (which build of the library ran: HORAYZON_HIP_LIB selects it).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.viewshed_perf import observers, terrain      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    from horayzon_amd.shadow import sight_heights
    n, off = args.tile, 16
    t, g, mask = terrain(n, off)
    shape = mask.shape
    dev = "cuda:%d" % t.device
    all_obs = observers(g, n, off, 16)
    obs = {16: torch.from_numpy(all_obs).to(dev), 1: torch.from_numpy(np.ascontiguousarray(all_obs[5:6])).to(dev)}
    tables = {129: sight_heights(256.05, 2.0), 1025: sight_heights(256.05, 0.25)}
    assert tables[129].size == 129 and tables[1025].size == 1025
    d_codes = torch.empty((16,) + shape, dtype=torch.uint8, device=dev)
    d_height = torch.empty((16,) + shape, dtype=torch.float32, device=dev)
    d_cells = torch.empty(16, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    passes = {}
    for S in (1, 16):
        for max_dist in (None, 5000.0):
            tag = "_S%d%s" % (S, "_5km" if max_dist else "")
            passes["viewshed" + tag] = (S, max_dist, lambda S=S, m=max_dist: t.viewshed(
                obs[S], visible=d_codes[:S], cells_seen=d_cells[:S], facing=False, target_elev=0.05, max_dist=m))
            for k in (129, 1025):
                passes["sight_%d%s" % (k, tag)] = (S, max_dist, lambda S=S, m=max_dist, k=k: t.sight_height(
                    obs[S], tables[k], height=d_height[:S], cells_reached=d_cells[:S], max_dist=m))

    kernel = {k: [] for k in passes}
    wall = {k: [] for k in passes}
    stats, reached = {}, {}
    for k, (_, _, fn) in passes.items():             # warm-up: code objects, staging buffers
        fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, (_, _, fn) in passes.items():
            t0 = time.perf_counter()
            fn()                                     # (every call ends in a stream synchronise of its own)
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
            kernel[k].append(t.last_stats["t_kernel_s"])
            stats[k] = dict(t.last_stats)
            reached[k] = int(d_cells[:passes[k][0]].sum().item())
    lines = []
    for k, (S, max_dist, _) in passes.items():
        med = statistics.median(kernel[k])
        rays = stats[k]["num_rays"]
        d = {"pass": k, "label": args.label, "tile": n, "observers": S, "max_dist": max_dist, "repeats": args.repeats,
             "t_kernel_ms_median": round(1e3 * med, 3), "t_kernel_ms_min": round(1e3 * min(kernel[k]), 3),
             "t_kernel_ms_max": round(1e3 * max(kernel[k]), 3), "ms_per_observer": round(1e3 * med / S, 4),
             "wall_ms_median": round(1e3 * statistics.median(wall[k]), 2), "num_rays": rays,
             "rays_per_observer": rays // S, "ns_per_ray": round(1e9 * med / max(rays, 1), 4),
             "cells_reached": reached[k], "scratch_bytes": stats[k]["scratch_bytes"]}
        lines.append(d)
        print(json.dumps(d), flush=True)
    by = {d["pass"]: d for d in lines}
    ratios = {"pass": "ratios", "label": args.label}
    for k, (S, max_dist, _) in passes.items():
        if k.startswith("sight"):
            base = by["viewshed_S%d%s" % (S, "_5km" if max_dist else "")]
            ratios[k + "_ns_per_ray_over_viewshed"] = round(by[k]["ns_per_ray"] / base["ns_per_ray"], 4)
            ratios[k + "_ms_over_viewshed"] = round(by[k]["ms_per_observer"] / base["ms_per_observer"], 4)
            ratios[k + "_rays_over_viewshed"] = round(by[k]["num_rays"] / max(base["num_rays"], 1), 4)
    lines.append(ratios)
    print(json.dumps(ratios), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
