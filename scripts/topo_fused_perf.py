"""Cost of the fused horizon reductions on the headline tile (3601^2, 360 azimuths, 50 km; the c3 workload of bench.py).

    python scripts/topo_fused_perf.py [--tile N] [--azim A] [--out FILE]
    python scripts/topo_fused_perf.py --c5 [--tile 14401] [--out FILE]

One warm-up and one timed step of each of
  - dev_svf:        the bench.py step: device-resident horizon + the SVF (k_topo<1>, hz_topo.hip)
  - dev_all:        the same + VSF and openness through hz_topo_out (k_topo<7>, one launch)
  - svf_only:       horizon never materialised (skip_hori), SVF only -- today's path for mosaics that do not fit
  - topo_only_all:  horizon never materialised, all three maps from one fused launch per chunk
  - separate_x3:    three hz_topo_params calls, one output each, on the materialised device horizon of dev_svf
  - params_fused:   one hz_topo_params call with all three outputs on the same horizon
and whether the fused maps equal the single-output ones bit for bit.  Kernel times of the horizon calls are
hz_stats.t_svf_s (HIP events); the hz_topo_params calls are timed on the host around a synchronising call.
--c5: config 5 instead (the 14401^2 mosaic, one call each through horizon_gridded, horizon never materialised): the
SVF alone (svf_only) and all three maps (topo_only).  Run it
under `rocprofv3 --kernel-trace --stats` for per-kernel times.  Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--dist-search", type=float, default=50.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--c5", action="store_true")
    args = ap.parse_args()
    if args.c5:
        return c5(args)
    import torch
    from horayzon_amd import _lib, synth
    L = _lib.lib()
    n, off, A = args.tile, 16, args.azim
    in0 = in1 = n - 2 * off
    g = synth.fractal_tile(n=n, offset=off)
    tilt_h, _ = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    sc = _lib.Scene.create(g["vert_grid"], n, n)
    dev = torch.device("cuda:0")
    d_norm = torch.zeros((in0, in1, 3), dtype=torch.float32, device=dev); d_norm[..., 2] = 1.0
    d_north = torch.zeros((in0, in1, 3), dtype=torch.float32, device=dev); d_north[..., 1] = 1.0
    d_mask = torch.ones((in0, in1), dtype=torch.uint8, device=dev)
    d_tilt = torch.from_numpy(tilt_h).to(dev)
    d_azim = torch.tensor([(2 * 3.141592653589793 / A) * i for i in range(A)], dtype=torch.float32).to(dev)
    d_hori = torch.empty((in0, in1, A), dtype=torch.float32, device=dev)

    def new_maps():
        return {k: torch.full((in0, in1), float("nan"), dtype=torch.float32, device=dev) for k in ("svf", "vsf", "openness")}

    def horizon(maps, names, skip):
        o = _lib.hz_opts()
        o.top_nodes, o.regroup = -1, -1
        o.vec_tilt = d_tilt.data_ptr()
        o.skip_hori = int(skip)
        o.svf = maps["svf"].data_ptr() if "svf" in names else None
        st = _lib.hz_stats()
        common = (sc._h, d_norm.data_ptr(), d_north.data_ptr(), off, off, None if skip else d_hori.data_ptr(), in0, in1, A,
                  args.dist_search, 0.25, b"guess_constant", -15.0, d_mask.data_ptr(), 0.0, 0.01, C.byref(o))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if "vsf" in names or "openness" in names:
            t = _lib.hz_topo_out(maps["vsf"].data_ptr() if "vsf" in names else None,
                                 maps["openness"].data_ptr() if "openness" in names else None)
            rc = L.hz_horizon_gridded_scene_ex(*common, C.byref(t), C.byref(st))
        else:
            rc = L.hz_horizon_gridded_scene(*common, C.byref(st))
        _lib.check(rc)
        torch.cuda.synchronize()
        return dict(step_s=time.perf_counter() - t0, t_svf_s=st.t_svf_s, t_kernel_s=st.t_kernel_s, t_near_s=st.t_near_s,
                    num_rays=int(st.num_rays))

    def params(maps, names):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.hz_topo_params(d_azim.data_ptr(), d_hori.data_ptr(), d_tilt.data_ptr(), in0, in1, A,
                                    maps["svf"].data_ptr() if "svf" in names else None,
                                    maps["vsf"].data_ptr() if "vsf" in names else None,
                                    maps["openness"].data_ptr() if "openness" in names else None, 0))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    all3 = ("svf", "vsf", "openness")
    res, maps = {}, {}
    for key, names, skip in (("svf_only", ("svf",), True), ("topo_only_all", all3, True),
                             ("dev_all", all3, False), ("dev_svf", ("svf",), False)):
        maps[key] = new_maps()
        horizon(maps[key], names, skip)                  # warm-up
        res[key] = horizon(maps[key], names, skip)
    # d_hori now holds the horizon of dev_svf's timed step: the reductions of a materialised horizon
    sep = new_maps()
    for name in all3:
        params(sep, (name,))
    res["separate_x3"] = {"s_" + name: params(sep, (name,)) for name in all3}
    res["separate_x3"]["total_s"] = sum(res["separate_x3"].values())
    fused = new_maps()
    params(fused, all3)
    res["params_fused"] = {"total_s": params(fused, all3)}
    same = {}
    for name in all3:
        ref = sep[name]
        same[name] = bool(torch.equal(fused[name], ref) and torch.equal(maps["dev_all"][name], ref)
                          and torch.equal(maps["topo_only_all"][name], ref))
    same["svf_paths"] = bool(torch.equal(maps["svf_only"]["svf"], sep["svf"]) and torch.equal(maps["dev_svf"]["svf"], sep["svf"]))
    out = {"tile": n, "azim": A, "dist_search_km": args.dist_search, "cells": in0 * in1,
           "device": torch.cuda.get_device_name(0), "rocm": getattr(torch.version, "hip", None),
           "results": res, "bit_identical": same}
    emit(out, args.out)
    sc.close()


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


def c5(args):
    import numpy as np
    from horayzon_amd import horizon, synth
    n = 14401 if args.tile == 3601 else args.tile
    off = 16
    g = synth.fractal_tile(n=n, offset=off)
    kw = {k: g[k] for k in ("vert_grid", "dem_dim_0", "dem_dim_1", "vec_norm", "vec_north", "offset_0", "offset_1")}
    tilt, _ = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    par = dict(dist_search=args.dist_search, azim_num=args.azim)
    res = {}
    t0 = time.perf_counter()
    _, _, svf = horizon.horizon_gridded(**kw, **par, svf_vec_tilt=tilt, svf_only=True)
    res["svf_only"] = dict(wall_s=time.perf_counter() - t0, **{k: horizon.last_stats[k] for k in ("t_kernel_s", "t_svf_s", "t_near_s")})
    t0 = time.perf_counter()
    _, _, maps = horizon.horizon_gridded(**kw, **par, topo=("svf", "vsf", "openness"), topo_vec_tilt=tilt, topo_only=True)
    res["topo_only_all"] = dict(wall_s=time.perf_counter() - t0, **{k: horizon.last_stats[k] for k in ("t_kernel_s", "t_svf_s", "t_near_s")})
    emit({"tile": n, "azim": args.azim, "cells": int(svf.size), "results": res, "svf_identical": bool(np.array_equal(svf, maps["svf"])),
          "nan_counts": {k: int(np.isnan(v).sum()) for k, v in maps.items()}}, args.out)


if __name__ == "__main__":
    main()
