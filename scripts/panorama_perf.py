"""Cost of Terrain.panorama on the c3 tile (synth.fractal_tile: 3601^2, offset 16): depth images of 3600 x 900 pixels
(azimuths over the full circle, elevations from straight down to straight up) from 1 and from 16 observers.

    python scripts/panorama_perf.py [--tile N] [--azim A] [--elev E] [--repeats R] [--out FILE]

After one warm-up of every pass, the passes are run R times in alternation; per pass the median kernel time of last_stats
(HIP events around the launches; for NumPy outputs the copies of the chunks lie inside them), its range, the wall time of a
call that ends in a device synchronise, ns per ray, ms per observer and the share of pixels with a hit.  Observers: the
summit (2 m above the highest vertex), the valley floor (2 m above the lowest vertex of the inner domain), 500 m above the
middle, and -- for the passes with 16 -- 13 more on a lattice, 2 - 10 m above the surface.  Passes:
  - one_summit, one_valley, one_above:  one observer, dist in HBM, 50 km
  - dist_hbm_50km, dist_hbm_1000km:     16 observers, dist in HBM, max_dist 50 km and 10^6 m
  - dist_point_hbm_50km:                dist and point in HBM
  - dist_numpy_50km, dist_point_numpy_50km: NumPy outputs (staged in chunks of observers, copied inside the chunk loop)
  - dist_hbm_50km_slot_order:           hz_debug_set("panorama_traversal", 0): hz_closest's slot order, same words
  - dist_hbm_50km_band:                 the same pixel count with the elevations within +-15 degrees of the horizontal
Prints one JSON line per pass and writes them to --out (default profiles/panorama/panorama_perf.jsonl, which holds a run on
an MI355X).  The comparison point is k_horidist's per-ray time (scripts/horidist_perf.py, "distance")."""
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

from scripts.viewshed_perf import observers as lattice_observers, terrain        # noqa: E402


def named_observers(g, n, off):
    x, y, z = g["x"], g["y"], g["z"]
    hi = np.unravel_index(np.argmax(z), z.shape)
    zi = z[off:n - off, off:n - off]
    lo = np.unravel_index(np.argmin(zi), zi.shape)
    lo = (lo[0] + off, lo[1] + off)
    mid = n // 2
    return np.array([[x[hi[1]], y[hi[0]], z[hi] + 2.0],
                     [x[lo[1]], y[lo[0]], z[lo] + 2.0],
                     [x[mid], y[mid], z[mid, mid] + 500.0]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--azim", type=int, default=3600)
    ap.add_argument("--elev", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama", "panorama_perf.jsonl"))
    args = ap.parse_args()
    import torch
    from horayzon_amd import _lib
    n, off, A, E = args.tile, 16, args.azim, args.elev
    t, g, mask = terrain(n, off)
    dev = "cuda:%d" % t.device
    three = named_observers(g, n, off)
    sixteen = np.ascontiguousarray(np.vstack([three, lattice_observers(g, n, off, 13)]), np.float32)
    S = sixteen.shape[0]
    azim = np.linspace(0.0, 2.0 * np.pi, A, endpoint=False).astype(np.float32)
    elev = np.linspace(-np.pi / 2, np.pi / 2, E).astype(np.float32)
    band = np.linspace(-np.pi / 12, np.pi / 12, E).astype(np.float32)
    d_obs = torch.from_numpy(sixteen).to(dev)
    d_dist = torch.empty((S, E, A), dtype=torch.float32, device=dev)
    d_point = torch.empty((S, E, A, 3), dtype=torch.float32, device=dev)
    d_hits = torch.empty(S, dtype=torch.int64, device=dev)
    h_dist = np.empty((S, E, A), np.float32)
    h_point = np.empty((S, E, A, 3), np.float32)
    torch.cuda.synchronize()

    def slot_order():
        _lib.check(_lib.lib().hz_debug_set(b"panorama_traversal", 0))
        try:
            t.panorama(d_obs, azim, elev, 5.0e4, dist=d_dist, hits=d_hits)
        finally:
            _lib.check(_lib.lib().hz_debug_set(b"panorama_traversal", -1))

    def one(k):
        return lambda: t.panorama(d_obs[k:k + 1], azim, elev, 5.0e4, dist=d_dist[k:k + 1], hits=d_hits[k:k + 1])

    passes = {
        "one_summit": (1, one(0)), "one_valley": (1, one(1)), "one_above": (1, one(2)),
        "dist_hbm_50km": (S, lambda: t.panorama(d_obs, azim, elev, 5.0e4, dist=d_dist, hits=d_hits)),
        "dist_hbm_1000km": (S, lambda: t.panorama(d_obs, azim, elev, 1.0e6, dist=d_dist, hits=d_hits)),
        "dist_point_hbm_50km": (S, lambda: t.panorama(d_obs, azim, elev, 5.0e4, dist=d_dist, point=d_point, hits=d_hits)),
        "dist_numpy_50km": (S, lambda: t.panorama(d_obs, azim, elev, 5.0e4, dist=h_dist, hits=d_hits)),
        "dist_point_numpy_50km": (S, lambda: t.panorama(d_obs, azim, elev, 5.0e4, dist=h_dist, point=h_point, hits=d_hits)),
        "dist_hbm_50km_slot_order": (S, slot_order),
        "dist_hbm_50km_band": (S, lambda: t.panorama(d_obs, azim, band, 5.0e4, dist=d_dist, hits=d_hits)),
    }
    kernel = {k: [] for k in passes}
    wall = {k: [] for k in passes}
    stats, hit_share, words = {}, {}, {}
    for k, (_, fn) in passes.items():            # warm-up: code objects, staging buffers
        fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, (num, fn) in passes.items():
            t0 = time.perf_counter()
            fn()                                 # (every call ends in a stream synchronise of its own)
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
            kernel[k].append(t.last_stats["t_kernel_s"])
            stats[k] = dict(t.last_stats)
            first = {"one_valley": 1, "one_above": 2}.get(k, 0)
            hit_share[k] = float(d_hits[first:first + num].sum().item()) / (num * E * A)
            if k in ("dist_hbm_50km", "dist_hbm_50km_slot_order"):
                words[k] = d_dist.view(torch.int32).clone()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for k, (num, _) in passes.items():
            med = statistics.median(kernel[k])
            d = {"pass": k, "tile": n, "azim_num": A, "elev_num": E, "observers": num, "repeats": args.repeats,
                 "t_kernel_ms_median": round(1e3 * med, 3), "t_kernel_ms_min": round(1e3 * min(kernel[k]), 3),
                 "t_kernel_ms_max": round(1e3 * max(kernel[k]), 3), "ms_per_observer": round(1e3 * med / num, 4),
                 "ns_per_ray": round(1e9 * med / stats[k]["num_rays"], 4), "wall_ms_median": round(1e3 * statistics.median(wall[k]), 2),
                 "num_rays": stats[k]["num_rays"], "hit_share": round(hit_share[k], 4), "scratch_bytes": stats[k]["scratch_bytes"],
                 "bvh_height": stats[k]["bvh_height"]}
            if k == "dist_hbm_50km_slot_order":
                d["equal"] = bool(torch.equal(words["dist_hbm_50km"], words[k]))
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
