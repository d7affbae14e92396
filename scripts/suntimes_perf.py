"""HorizonTerrain.sun_times on the c3 tile (3601^2, 360 azimuths, the 144 sun positions of synth.sun_positions with uniform
times), everything resident in HBM, against HorizonTerrain.accumulate(sunlit_sum=...) of the same object and positions in
the same process.

    python scripts/suntimes_perf.py [--tile N] [--suns S] [--azim A] [--passes P] [--out FILE]

The tile's own horizon (guess_constant, dist_search 50 km, hori_acc 0.25 deg) is computed into a torch tensor in HBM and
borrowed by a cell-major HorizonTerrain; hz_hori_to_planes makes the planes a second object borrows.  For each layout, without
and with refraction(elevation): one warm-up, then P passes of the two calls alternating; one JSON line per (layout, refrac,
call) with the median kernel time per position (HIP events around the launches, last_stats["t_kernel_s"]), the median wall
time per position and scratch_bytes.  The four maps of the two layouts are compared word for word on the whole tile."""
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
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--suns", type=int, default=144)
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--dist-search", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes as C
    import torch
    import horayzon_amd as hz
    from horayzon_amd import _lib, synth
    from horayzon_amd.shadow import gridded_azimuths
    if _lib.device_count() < 1:
        raise SystemExit("suntimes_perf.py needs an MI355X")
    n, off, A = args.tile, 16, args.azim
    g = synth.fractal_tile(n=n, offset=off)
    in0 = in1 = n - 2 * off
    vec_tilt, enl = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    vec_norm, vec_north = synth.planar_frames(in0, in1)
    elev = np.ascontiguousarray(g["z"][off:off + in0, off:off + in1], np.float32)
    mask = np.ones((in0, in1), np.uint8)
    suns, _, _ = synth.sun_positions(num=args.suns)
    S = suns.shape[0]
    times = np.linspace(0.0, 24.0, S, endpoint=False)
    shape = mask.shape
    dev = "cuda:0"
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    L = _lib.lib()
    scene = hz.Scene.create(g["vert_grid"], n, n)
    d_hori = torch.empty((in0, in1, A), dtype=torch.float32, device=dev)
    d_mask = torch.from_numpy(mask).to(dev)
    torch.cuda.synchronize()
    opts = _lib.hz_opts()
    opts.device, opts.top_nodes, opts.regroup = 0, -1, -1
    st = _lib.hz_stats()
    _lib.check(L.hz_horizon_gridded_scene(scene._h, _lib.ptr(vec_norm), _lib.ptr(vec_north), off, off, d_hori.data_ptr(),
                                          in0, in1, A, args.dist_search, 0.25, b"guess_constant", -15.0, d_mask.data_ptr(),
                                          0.0, 0.01, C.byref(opts), C.byref(st)))
    emit({"figure": "horizon", "tile": n, "azim_num": A, "t_kernel_ms": round(1e3 * st.t_kernel_s, 1)})
    d_planes = torch.empty((A, in0, in1), dtype=torch.float32, device=dev)
    _lib.check(L.hz_hori_to_planes(d_hori.data_ptr(), in0, in1, A, d_planes.data_ptr(), 0))
    torch.cuda.synchronize()

    objs = {}
    for layout, hori in (("cell_major", d_hori), ("azim_major", d_planes)):
        t = hz.shadow.HorizonTerrain()
        (t.initialise_azim_major if layout == "azim_major" else t.initialise)(
            gridded_azimuths(A), hori, g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, vec_north, enl, mask,
            sw_dir_cor_fill=-7.0)
        objs[layout] = t
    d_suns = torch.from_numpy(suns).to(dev)
    maps = {layout: dict(sunrise=torch.empty(shape, dtype=torch.float32, device=dev),
                         sunset=torch.empty(shape, dtype=torch.float32, device=dev),
                         duration=torch.empty(shape, dtype=torch.float32, device=dev),
                         intervals=torch.empty(shape, dtype=torch.int32, device=dev)) for layout in objs}
    d_lit = torch.empty(shape, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    for refrac in (False, True):
        for layout, t in objs.items():
            t.refraction(elev if refrac else None)
            calls = {"sun_times": lambda: t.sun_times(d_suns, times, **maps[layout]),
                     "accumulate": lambda: t.accumulate(d_suns, None, sunlit_sum=d_lit)}
            kernel = {k: [] for k in calls}
            wall = {k: [] for k in calls}
            scratch = {}
            for p in range(args.passes + 1):                       # pass 0 warms up
                for name, fn in calls.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if p:
                        wall[name].append(time.perf_counter() - t0)
                        kernel[name].append(t.last_stats["t_kernel_s"])
                        scratch[name] = t.last_stats["scratch_bytes"]
            for name in calls:
                emit({"figure": "speed", "call": name, "layout": layout, "refrac": refrac, "tile": n, "suns": S,
                      "kernel_ms_per_position": round(1e3 * float(np.median(kernel[name])) / S, 4),
                      "wall_ms_per_position": round(1e3 * float(np.median(wall[name])) / S, 4),
                      "scratch_bytes": int(scratch[name]), "passes": args.passes})
        a, b = maps["cell_major"], maps["azim_major"]
        emit({"figure": "layouts_equal", "refrac": refrac,
              "equal": all(bool(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))) for k in a),
              "cells_never_lit": int((a["intervals"] == 0).sum()), "max_intervals": int(a["intervals"].max()),
              "mean_duration": round(float(a["duration"].double().mean()), 4)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
