"""The distance to the horizon (DESIGN.md section 4 clause 16, hz_horidist.hip) on the c3 tile (3601^2, 360 azimuths): what
the distance pass costs next to the horizon step of the same run, and against the closest-hit path that was there before.

    python scripts/horidist_perf.py [--tile N] [--azim A] [--passes P] [--sample S] [--out FILE]

Everything is resident in HBM (torch tensors), times are the library's kernel times (device events, hz_stats.t_kernel_s).
One warm-up, then P = 3 timed passes per variant, the variants of an A/B alternating; one JSON line per figure (default
FILE: profiles/horidist/horidist_perf.jsonl):
  "horizon":   the horizon step (guess_constant) into HBM: kernel ms, rays, Gray/s.
  "distance":  the stand-alone distance pass on that horizon, cell-major: kernel ms (median, min, max) and closest-hit rays
               per second with the children of a node front to back ("traversal": 1, the default) and with hz_closest as it
               is (0), same call, alternating; the share of the horizon step; "equal": both give the same words.
  "distance_planes": the same on planes with blocks of 8 x 8 cells (the default) and of 32 x 2 ("block_w").
  "distance_q16": from 16-bit codes, cell-major.
  "gridded_dist": hz_horizon_gridded_scene_dist into HBM: kernel ms of horizon + distances in one call.
  "host_copy": the NumPy-out call horizon_gridded(hori_dist=True) on a slab of rows: wall seconds and t_d2h_s with and
               without distances (the distance chunks are copied inside the chunk loop, not overlapped).
  "locations": the yardstick -- horizon_locations(hori_dist_out=True, ray_algorithm="binary_search") on a strided sample
               of S x S of the same cells: kernel ns per closest-hit ray, next to the distance pass's."""
import argparse
import ctypes as C
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
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--dist-search", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--sample", type=int, default=192, help="the yardstick runs on SAMPLE x SAMPLE cells of the window")
    ap.add_argument("--host-rows", type=int, default=256, help="rows of the NumPy-out call (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "horidist", "horidist_perf.jsonl"))
    args = ap.parse_args()
    import torch
    import horayzon_amd as hz
    from horayzon_amd import _lib, synth
    H = hz.horizon
    n, off, A = args.tile, 16, args.azim
    g = synth.fractal_tile(n=n, offset=off)
    in0 = in1 = n - 2 * off
    vec_norm, vec_north = synth.planar_frames(in0, in1)
    mask = np.ones((in0, in1), np.uint8)
    dev = "cuda:0"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out_file = open(args.out, "w")

    def emit(d):
        d = dict(d, tile=n, azim_num=A)
        print(json.dumps(d), flush=True)
        out_file.write(json.dumps(d) + "\n")
        out_file.flush()

    L = _lib.lib()
    scene = hz.Scene.create(g["vert_grid"], n, n)
    d_norm, d_north = torch.from_numpy(vec_norm).to(dev), torch.from_numpy(vec_north).to(dev)
    d_mask = torch.from_numpy(mask).to(dev)
    hori = torch.empty((in0, in1, A), dtype=torch.float32, device=dev)
    dist = {k: torch.empty((in0, in1, A), dtype=torch.float32, device=dev) for k in (0, 1)}
    torch.cuda.synchronize()
    opts = _lib.hz_opts()
    opts.device, opts.top_nodes, opts.regroup = 0, -1, -1
    rays_total = in0 * in1 * A

    def horizon_call(dist_buf=None):
        st = _lib.hz_stats()
        head = (scene._h, d_norm.data_ptr(), d_north.data_ptr(), off, off, hori.data_ptr())
        tail = (in0, in1, A, args.dist_search, 0.25, b"guess_constant", -15.0, d_mask.data_ptr(), 0.0, 0.01, C.byref(opts))
        if dist_buf is None:
            _lib.check(L.hz_horizon_gridded_scene(*head, *tail, C.byref(st)))
        else:
            _lib.check(L.hz_horizon_gridded_scene_dist(*head, 0, dist_buf.data_ptr(), *tail, None, C.byref(st)))
        return st.as_dict()

    def distance_call(src, kind, dst):
        st = _lib.hz_stats()
        _lib.check(L.hz_horizon_distance_scene(scene._h, src.data_ptr(), kind, dst.data_ptr(), d_norm.data_ptr(), d_north.data_ptr(),
                                               off, off, in0, in1, A, args.dist_search, 0.25, -15.0, d_mask.data_ptr(), 0.01,
                                               C.byref(opts), C.byref(st)))
        return st.as_dict()

    def stat(ms):
        ms = sorted(ms)
        return dict(kernel_ms=round(ms[len(ms) // 2], 1), kernel_ms_min_max=[round(ms[0], 1), round(ms[-1], 1)],
                    grays_per_s=round(rays_total / (ms[len(ms) // 2] * 1e-3) / 1e9, 3))

    def same(a, b):
        return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))

    def ab(figure, knob, values, src, kind, shape_of=lambda t: t, extra=None):
        """variants `values` of hz_debug_set(knob), alternating: one warm-up each, then the timed passes"""
        ms = {v: [] for v in values}
        for p in range(args.passes + 1):
            for i, v in enumerate(values):
                _lib.check(L.hz_debug_set(knob, v))
                st = distance_call(src, kind, shape_of(dist[i]))
                if p:
                    ms[v].append(1e3 * st["t_kernel_s"])
        _lib.check(L.hz_debug_set(knob, -1))
        eq = all(same(dist[0], dist[i]) for i in range(1, len(values)))
        for v in values:
            emit(dict({"figure": figure, knob.decode().replace("horidist_", ""): v, "rays": rays_total, "equal": eq,
                       "share_of_horizon_step": round(sorted(ms[v])[len(ms[v]) // 2] / hori_ms, 3)}, **stat(ms[v]), **(extra or {})))
        return ms

    # the horizon step
    horizon_call()
    h_ms = []
    for _ in range(args.passes):
        st = horizon_call()
        h_ms.append(1e3 * st["t_kernel_s"])
    hori_ms = sorted(h_ms)[len(h_ms) // 2]
    emit({"figure": "horizon", "kernel_ms": round(hori_ms, 1), "kernel_ms_min_max": [round(min(h_ms), 1), round(max(h_ms), 1)],
          "rays": int(st["num_rays"]), "grays_per_s": round(st["num_rays"] / (hori_ms * 1e-3) / 1e9, 3)})
    nan_share = float(torch.isnan(hori).float().mean())

    # the distance pass, cell-major: front to back against hz_closest's order
    ms = ab("distance", b"horidist_traversal", (1, 0), hori, 0)
    dist_ms = sorted(ms[1])[len(ms[1]) // 2]
    emit({"figure": "distance_nan_share", "horizon": nan_share, "distance": float(torch.isnan(dist[0]).float().mean())})
    ref_planes = dist[0].permute(2, 0, 1).contiguous()

    # planes: blocks of 8 x 8 against 32 x 2
    planes = hori.permute(2, 0, 1).contiguous()
    ab("distance_planes", b"horidist_block_w", (8, 32), planes, 1, shape_of=lambda t: t.view(A, in0, in1))
    emit({"figure": "distance_planes_equal", "equal": same(dist[0].view(A, in0, in1), ref_planes)})
    del planes, ref_planes

    # from codes
    q = torch.empty((in0, in1, A), dtype=torch.int16, device=dev)
    _lib.check(L.hz_hori_quantise(hori.data_ptr(), hori.numel(), q.data_ptr(), 0))
    q_ms = []
    for p in range(args.passes + 1):
        st = distance_call(q, 2, dist[1])
        if p:
            q_ms.append(1e3 * st["t_kernel_s"])
    emit(dict({"figure": "distance_q16", "rays": rays_total}, **stat(q_ms)))
    del q

    # horizon and distances in one call
    g_ms = []
    for p in range(args.passes + 1):
        st = horizon_call(dist[1])
        if p:
            g_ms.append(1e3 * st["t_kernel_s"])
    distance_call(hori, 0, dist[0])
    emit({"figure": "gridded_dist", "kernel_ms": round(sorted(g_ms)[len(g_ms) // 2], 1),
          "kernel_ms_min_max": [round(min(g_ms), 1), round(max(g_ms), 1)], "horizon_ms": round(hori_ms, 1),
          "distance_ms": round(dist_ms, 1), "equal": same(dist[0], dist[1])})

    # the yardstick: the closest-hit path of horizon_locations on a sample of the same cells
    S = min(args.sample, in0)
    idx = np.linspace(0, in0 - 1, S).astype(np.int64)
    verts = g["vert_grid"][:3 * n * n].reshape(n, n, 3)
    coords = np.ascontiguousarray(verts[off + idx][:, off + idx].reshape(-1, 3))
    ln, lnorth = np.zeros_like(coords), np.zeros_like(coords)
    ln[:, 2], lnorth[:, 1] = 1.0, 1.0
    l_ns = []
    for p in range(args.passes + 1):
        H.horizon_locations(g["vert_grid"], n, n, coords, ln, lnorth, args.dist_search, azim_num=A, ray_algorithm="binary_search",
                            elev_ang_low_lim=-15.0, hori_dist_out=True, scene=scene)
        st = H.last_stats
        if p:
            l_ns.append(1e9 * st["t_kernel_s"] / st["num_rays"])
    l_ns.sort()
    emit({"figure": "locations", "cells": int(S * S), "rays": int(st["num_rays"]), "rays_per_cell_and_azimuth": round(st["num_rays"] / (S * S * A), 2),
          "kernel_ns_per_ray": round(l_ns[len(l_ns) // 2], 3), "kernel_ns_per_ray_min_max": [round(l_ns[0], 3), round(l_ns[-1], 3)],
          "distance_pass_ns_per_ray": round(1e6 * dist_ms / rays_total, 3)})
    del dist, hori
    torch.cuda.empty_cache()

    # NumPy out on a slab of rows: what the distance chunks cost in copies (not overlapped with the next chunk's tracing)
    if args.host_rows > 0:
        r0 = (in0 - args.host_rows) // 2
        hr = args.host_rows         # (an inner domain of its own: the middle rows of the window)
        kw = dict(vert_grid=g["vert_grid"], dem_dim_0=n, dem_dim_1=n, vec_norm=vec_norm[:hr], vec_north=vec_north[:hr],
                  offset_0=off + r0, offset_1=off, dist_search=args.dist_search, azim_num=A, mask=mask[:hr], scene=scene)
        for flag in (False, True):
            walls, sts = [], []
            for p in range(2):
                t0 = time.perf_counter()
                H.horizon_gridded(**kw, hori_dist=flag)
                walls.append(time.perf_counter() - t0)
                sts.append(dict(H.last_stats))
            emit({"figure": "host_copy", "hori_dist": flag, "rows": args.host_rows, "wall_s": round(min(walls), 3),
                  "t_kernel_s": round(sts[-1]["t_kernel_s"], 3), "t_d2h_s": round(sts[-1]["t_d2h_s"], 3),
                  "bytes_per_array": args.host_rows * in1 * A * 4})
    scene.close()


if __name__ == "__main__":
    main()
