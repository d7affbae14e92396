"""Cost of Terrain.viewshed on the c3 tile (synth.fractal_tile: 3601^2, offset 16) for 16 observers a few metres above
cells spread over the tile, against shadow_batch for 16 sun positions -- the existing kernel on the same box, in the same
process.

    python scripts/viewshed_perf.py [--tile N] [--observers S] [--repeats R] [--out FILE]

Everything is device resident (observers, sun positions and outputs are torch tensors in HBM).  After one warm-up of every
pass, the passes are run R times in alternation; per pass the median kernel time of last_stats (HIP events around the
launches), its range, and the wall time of a call that ends in a device synchronise.  Passes:
  - shadow_batch:     shadow_batch of S sun positions of synth.sun_positions(num=144), evenly spaced (night included)
  - shadow_batch_day: the same for the S positions that trace the most rays
  - viewshed_codes:   viewshed(visible=...)
  - viewshed_counts:  viewshed(seen_count=..., cells_seen=...): no map per observer, one atomic per visible cell
  - viewshed_all:     all three outputs
  - viewshed_back:    viewshed(visible=..., facing=False): a ray for every cell
  - viewshed_5km:     viewshed(visible=..., max_dist=5000)
Prints one JSON line per pass, then the ratios of the per-observer time to shadow_batch's per-position time, and writes
them to --out (profiles/viewshed/viewshed_perf.jsonl holds a run on an MI355X).
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


def terrain(n, off=16):
    import horayzon_amd as hz
    from horayzon_amd import synth
    g = synth.fractal_tile(n=n, offset=off)
    in0 = in1 = n - 2 * off
    vec_tilt, enl = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    vec_norm, _ = synth.planar_frames(in0, in1)
    elev = np.ascontiguousarray(g["z"][off:off + in0, off:off + in1], np.float32)
    mask = np.ones((in0, in1), np.uint8)
    t = hz.shadow.Terrain()
    t.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask)
    return t, g, mask


def observers(g, n, off, num):
    """`num` points 2 - 10 m above DEM vertices on a regular lattice over the inner domain."""
    side = int(np.ceil(np.sqrt(num)))
    at = (off + (np.arange(side) + 0.5) * (n - 2 * off) / side).astype(int)
    ii, jj = [a.ravel()[:num] for a in np.meshgrid(at, at, indexing="ij")]
    height = np.linspace(2.0, 10.0, num)
    return np.ascontiguousarray(np.stack([g["x"][jj], g["y"][ii], g["z"][ii, jj] + height], axis=1), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--observers", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from horayzon_amd import synth
    n, S, off = args.tile, args.observers, 16
    t, g, mask = terrain(n, off)
    shape = mask.shape
    dev = "cuda:%d" % t.device
    obs = torch.from_numpy(observers(g, n, off, S)).to(dev)
    all_suns, _, _ = synth.sun_positions(num=144)
    d_codes = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
    d_seen = torch.empty(shape, dtype=torch.int32, device=dev)
    d_cells = torch.empty(S, dtype=torch.int64, device=dev)
    # the S positions of the day with the most rays: one call over all 144 would need 1.8 GB; rays per position from single calls
    rays = []
    one = torch.empty((1,) + shape, dtype=torch.uint8, device=dev)
    for s in range(0, 144, 3):
        t.shadow_batch(np.ascontiguousarray(all_suns[s:s + 1]), one)
        rays.append((t.last_stats["num_rays"], s))
    day = sorted(s for _, s in sorted(rays, reverse=True)[:S])
    suns = torch.from_numpy(np.ascontiguousarray(all_suns[::144 // S][:S])).to(dev)
    suns_day = torch.from_numpy(np.ascontiguousarray(all_suns[day])).to(dev)
    torch.cuda.synchronize()

    def batch(positions):
        # (shadow_batch takes its positions as a NumPy array; the library call below is the one it makes, with positions in HBM)
        import ctypes as C
        from horayzon_amd import _lib
        st = _lib.hz_stats()
        _lib.check(_lib.lib().hz_terrain_shadow_batch(t._h, _lib.ptr(positions), positions.shape[0], _lib.ptr(d_codes), C.byref(st)))
        t.last_stats = st.as_dict()

    passes = {
        "shadow_batch": lambda: batch(suns),
        "shadow_batch_day": lambda: batch(suns_day),
        "viewshed_codes": lambda: t.viewshed(obs, visible=d_codes),
        "viewshed_counts": lambda: t.viewshed(obs, seen_count=d_seen, cells_seen=d_cells),
        "viewshed_all": lambda: t.viewshed(obs, visible=d_codes, seen_count=d_seen, cells_seen=d_cells),
        "viewshed_back": lambda: t.viewshed(obs, visible=d_codes, facing=False),
        "viewshed_5km": lambda: t.viewshed(obs, visible=d_codes, max_dist=5000.0),
    }

    kernel = {k: [] for k in passes}
    wall = {k: [] for k in passes}
    stats = {}
    for k, fn in passes.items():             # warm-up: code objects, staging buffers
        fn()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, fn in passes.items():
            t0 = time.perf_counter()
            fn()                             # (every call ends in a stream synchronise of its own)
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
            kernel[k].append(t.last_stats["t_kernel_s"])
            stats[k] = dict(t.last_stats)
    lines = []
    for k in passes:
        med = statistics.median(kernel[k])
        d = {"pass": k, "tile": n, "positions": S, "repeats": args.repeats,
             "t_kernel_ms_median": round(1e3 * med, 3), "t_kernel_ms_min": round(1e3 * min(kernel[k]), 3),
             "t_kernel_ms_max": round(1e3 * max(kernel[k]), 3), "ms_per_position": round(1e3 * med / S, 4),
             "wall_ms_median": round(1e3 * statistics.median(wall[k]), 2), "num_rays": stats[k]["num_rays"],
             "rays_per_position": stats[k]["num_rays"] // S, "scratch_bytes": stats[k]["scratch_bytes"]}
        lines.append(d)
        print(json.dumps(d), flush=True)
    per = {d["pass"]: d["ms_per_position"] for d in lines}
    ratios = {"pass": "ratios", "cells_seen": [int(v) for v in d_cells.cpu().numpy()]}
    for k in passes:
        if k.startswith("viewshed"):
            ratios[k + "_over_shadow_batch"] = round(per[k] / per["shadow_batch"], 4)
            ratios[k + "_over_shadow_batch_day"] = round(per[k] / per["shadow_batch_day"], 4)
    lines.append(ratios)
    print(json.dumps(ratios), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
