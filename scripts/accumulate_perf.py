"""Cost of Terrain.accumulate on the c3 tile (3601^2, the 144 sun positions of synth.sun_positions), against the
per-position batch calls it replaces.

    python scripts/accumulate_perf.py [--tile N] [--out FILE]
    python scripts/accumulate_perf.py --mosaic [--out FILE]

One warm-up and one timed pass of each of
  - shadow_batch_hbm:      shadow_batch into a torch u8 [144][y][x] tensor in HBM
  - sw_dir_cor_batch_hbm:  sw_dir_cor_batch into a torch f32 [144][y][x] tensor in HBM
  - accumulate_both:       accumulate, sw_dir_cor_sum and sunlit_sum (NumPy outputs)
  - accumulate_sw:         accumulate, sw_dir_cor_sum only (NumPy output)
  - batch_numpy_host_sum:  sw_dir_cor_batch into NumPy and a float64 host sum, ascending -- the end-to-end form without
                           accumulate
For each: the kernel time from last_stats (HIP events), the wall time, scratch_bytes and whether the maps are
bit-identical to the float64 ascending reduction of the batch maps.  --mosaic: the 14401^2 tile instead, accumulate only
(both outputs, then sw_dir_cor_sum only).  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel times.
Prints one JSON line per pass (and writes them to --out).
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
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--suns", type=int, default=144)
    ap.add_argument("--mosaic", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from horayzon_amd import synth
    n = 14401 if args.mosaic else args.tile
    t, mask = terrain(n)
    suns, _, _ = synth.sun_positions(num=args.suns)
    S = suns.shape[0]
    w = np.full(S, 600.0, np.float32)                # 10-minute steps in seconds
    shape = mask.shape
    lines = []

    def report(name, stats, wall, identical=None):
        d = {"pass": name, "tile": n, "suns": S, "t_kernel_ms": round(1e3 * stats["t_kernel_s"], 3),
             "wall_ms": round(1e3 * wall, 1), "num_rays": stats["num_rays"], "scratch_bytes": stats["scratch_bytes"],
             "identical": identical}
        lines.append(d)
        print(json.dumps(d), flush=True)

    def acc(sw=True, lit=True):
        o_sw = np.empty(shape, np.float32) if sw else None
        o_lit = np.empty(shape, np.float32) if lit else None
        t.accumulate(suns, w, sw_dir_cor_sum=o_sw, sunlit_sum=o_lit)
        return o_sw, o_lit, dict(t.last_stats)

    if not args.mosaic:
        dev = "cuda:%d" % t.device
        w_dev = torch.from_numpy(w.astype(np.float64)).to(dev)
        m_dev = torch.from_numpy(mask).to(dev) != 1

        # the yardsticks, reduced on the GPU in float64, ascending s (elementwise float64 ops: the same sums as NumPy's)
        d_sh = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
        _, wall = timed(lambda: t.shadow_batch(suns, d_sh))
        st_sh = dict(t.last_stats)
        torch.cuda.synchronize()
        ref_lit = torch.zeros(shape, dtype=torch.float64, device=dev)
        for s in range(S):
            ref_lit += w_dev[s] * (d_sh[s] == 0).double()
        ref_lit = ref_lit.float().masked_fill_(m_dev, -7.0).cpu().numpy()
        report("shadow_batch_hbm", st_sh, wall)
        del d_sh
        torch.cuda.empty_cache()

        d_sw = torch.empty((S,) + shape, dtype=torch.float32, device=dev)
        _, wall = timed(lambda: t.sw_dir_cor_batch(suns, d_sw))
        st_sw = dict(t.last_stats)
        torch.cuda.synchronize()
        ref_sw = torch.zeros(shape, dtype=torch.float64, device=dev)
        for s in range(S):
            ref_sw += w_dev[s] * d_sw[s].double()
        ref_sw = ref_sw.float().masked_fill_(m_dev, -7.0).cpu().numpy()
        report("sw_dir_cor_batch_hbm", st_sw, wall)
        del d_sw
        torch.cuda.empty_cache()

        (a_sw, a_lit, st), wall = timed(lambda: acc())
        report("accumulate_both", st, wall, bool(np.array_equal(a_sw, ref_sw) and np.array_equal(a_lit, ref_lit)))
        (a_sw, _, st), wall = timed(lambda: acc(lit=False))
        report("accumulate_sw", st, wall, bool(np.array_equal(a_sw, ref_sw)))

        def host_sum():
            maps = np.empty((S,) + shape, np.float32)
            t.sw_dir_cor_batch(suns, maps)
            st = dict(t.last_stats)
            total = np.zeros(shape)
            w64 = w.astype(np.float64)
            for s in range(S):
                total += w64[s] * maps[s].astype(np.float64)
            out = total.astype(np.float32)
            out[mask != 1] = -7.0
            return out, st
        (h_sw, st), wall = timed(host_sum)
        report("batch_numpy_host_sum", st, wall, bool(np.array_equal(h_sw, ref_sw)))
        both = next(d for d in lines if d["pass"] == "accumulate_both")
        print(json.dumps({"accumulate_both_over_shadow_batch": round(both["t_kernel_ms"] / lines[0]["t_kernel_ms"], 4),
                          "host_sum_wall_over_accumulate_wall": round(lines[-1]["wall_ms"] / both["wall_ms"], 2)}))
    else:
        (_, _, st), wall = timed(lambda: acc())
        report("accumulate_both", st, wall)
        (_, _, st), wall = timed(lambda: acc(lit=False))
        report("accumulate_sw", st, wall)
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
