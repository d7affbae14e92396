"""Cost of Terrain.sw_dir_cor_coarse on the c3 tile (3601^2, 3569^2 inner cells, the 144 sun positions of
synth.sun_positions) with 43 x 43 cells per coarse cell (83 x 83 coarse cells), against the calls it stands beside.

    python scripts/coarse_perf.py [--small] [--out FILE]

One warm-up and one timed pass of each of, in one process,
  - sw_dir_cor_batch_hbm:  sw_dir_cor_batch into a torch f32 [S][y][x] tensor in HBM (and shadow_batch into a u8 one: the
                           maps the yardstick is reduced from, on the GPU, in the contract's order)
  - coarse_both:           sw_dir_cor_coarse, f_cor and sunlit_frac (NumPy outputs)
  - coarse_f_cor:          sw_dir_cor_coarse, f_cor only
  - accumulate_both:       accumulate, sw_dir_cor_sum and sunlit_sum (NumPy outputs): the same chunks traced, another reduction
For each: wall time, the kernel time from last_stats (HIP events), scratch_bytes, num_rays; for the coarse passes whether the
tables are bit-identical to the yardstick.  Prints ONE JSON line (and appends it to --out).  --small: a 376^2 tile (8 x 8 coarse
cells) and 24 positions, seconds.  Run it under `rocprofv3 --kernel-trace --stats` for the share of k_coarse_reduce and
k_accum_add.
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
    t.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-7.0)
    return t, mask


def timed(fn):
    """One warm-up, one timed pass: (result of the timed pass, its wall seconds)."""
    fn()
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from horayzon_amd import synth
    P = 43
    n, S = (376, 24) if args.small else (3601, 144)
    t, mask = terrain(n)
    suns, _, _ = synth.sun_positions(num=S)
    shape = mask.shape
    gy, gx = shape[0] // P, shape[1] // P
    line = {"tile": n, "suns": S, "pixel_per_gc": P, "coarse_cells": [gy, gx]}

    def entry(stats, wall, identical=None):
        d = {"wall_s": round(wall, 4), "t_kernel_s": round(stats["t_kernel_s"], 6), "scratch_bytes": stats["scratch_bytes"],
             "num_rays": stats["num_rays"]}
        if identical is not None:
            d["identical"] = identical
        return d

    # the batch maps in HBM, and from them the yardstick: float64, the block's cells in row-major order, one rounding (the
    # mask is all ones here; elementwise float64 adds on the GPU are the same sums as NumPy's).  The division is NumPy's:
    # torch divides by a scalar as a product with its reciprocal, which is not the correctly rounded quotient
    dev = "cuda:%d" % t.device
    d_sh = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
    t.shadow_batch(suns, d_sh)
    torch.cuda.synchronize()
    lit = (d_sh == 0).view(S, gy, P, gx, P).sum(dim=(2, 4))
    ref_lit = (lit.cpu().numpy().astype(np.float64) / float(P * P)).astype(np.float32)
    del d_sh, lit
    torch.cuda.empty_cache()
    d_sw = torch.empty((S,) + shape, dtype=torch.float32, device=dev)
    _, wall = timed(lambda: (t.sw_dir_cor_batch(suns, d_sw), torch.cuda.synchronize()))
    line["sw_dir_cor_batch_hbm"] = entry(dict(t.last_stats), wall)
    line["sw_dir_cor_batch_hbm"]["map_bytes"] = d_sw.numel() * 4
    acc = torch.zeros((S, gy, gx), dtype=torch.float64, device=dev)
    for di in range(P):
        for dj in range(P):
            acc += d_sw[:, di::P, dj::P].double()
    ref_f = (acc.cpu().numpy() / float(P * P)).astype(np.float32)
    del d_sw, acc
    torch.cuda.empty_cache()

    def coarse(sw=True, lit=True):
        f_cor = np.empty((S, gy, gx), np.float32) if sw else None
        frac = np.empty((S, gy, gx), np.float32) if lit else None
        t.sw_dir_cor_coarse(suns, P, f_cor=f_cor, sunlit_frac=frac)
        return f_cor, frac, dict(t.last_stats)

    def accumulate():
        o_sw, o_lit = np.empty(shape, np.float32), np.empty(shape, np.float32)
        t.accumulate(suns, sw_dir_cor_sum=o_sw, sunlit_sum=o_lit)
        return dict(t.last_stats)

    (f_cor, frac, st), wall = timed(coarse)
    line["coarse_both"] = entry(st, wall, bool(np.array_equal(f_cor, ref_f) and np.array_equal(frac, ref_lit)))
    line["coarse_both"]["table_bytes"] = f_cor.nbytes + frac.nbytes
    (f_cor, _, st), wall = timed(lambda: coarse(lit=False))
    line["coarse_f_cor"] = entry(st, wall, bool(np.array_equal(f_cor, ref_f)))
    st, wall = timed(accumulate)
    line["accumulate_both"] = entry(st, wall)
    line["coarse_both_over_accumulate_both_kernel"] = round(line["coarse_both"]["t_kernel_s"] / line["accumulate_both"]["t_kernel_s"], 4)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
