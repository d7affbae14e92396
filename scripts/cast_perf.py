"""Cost of Terrain.cast on the c3 tile (synth.fractal_tile: 3601^2, offset 16), against the calls whose rays it restates.

    python scripts/cast_perf.py [--tile N] [--azim A] [--elev E] [--observers S] [--repeats R] [--out FILE]

After one warm-up of every pass, the passes are run R times in alternation; per pass the median kernel time of last_stats
(HIP events around the launches; for NumPy arrays the copies of the chunks lie inside them), its range, the wall time of a
call that ends in a device synchronise (for cast it holds the finiteness and unit-length reductions of the tensors), ns per
ray and the share of rays with a hit.  Passes:
  (a) panorama            Terrain.panorama, S observers (scripts/panorama_perf.py's 16), A x E pixels, dist in HBM, 50 km
      cast_image          the same rays as explicit device-resident origins and directions in image order, dist in HBM
      cast_image_any      the same, occluded alone (the any-hit kernel)
  (b) cast_shuffled_given the same rays in a random permutation, order="given"
      cast_shuffled_sorted   ... order="sorted": keys, sort and tracing
      cast_shuffled_sort_only   ... hz_debug_set("cast_sort_only", 1): keys and sort alone
      cast_image_sorted   image order with order="sorted": what the sort costs rays that need none
      cast_image_tiled    the rays in panorama's wave shape: tiles of 8 elevations x 8 azimuths, 64 consecutive rays each
  (c) viewshed            Terrain.viewshed(facing=False), one observer (the summit), codes in HBM
      cast_segments       its segments (target point of every cell -> the observer) as cast(targets=...), occluded alone
      cast_segments_dist  the same with dist (the closest-hit kernel)
      cast_segments_shuffled_given / _sorted, cast_segments_dist_shuffled_given / _sorted
                          the segments in a random permutation (12.7 M different origins), both kernels, both orders
  (d) cast_image_numpy    (a)'s cast from NumPy origins and directions into a NumPy dist
The directions here are float32 roundings of float64 trigonometry, not panorama's table products: the two calls trace rays
that differ in the last bits, which the times do not see.  Prints one JSON line per pass and writes them to --out (default
profiles/cast/cast_perf.jsonl, which holds a run on an MI355X)."""
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

from scripts.panorama_perf import named_observers                                # noqa: E402
from scripts.viewshed_perf import observers as lattice_observers, terrain        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--azim", type=int, default=3600)
    ap.add_argument("--elev", type=int, default=900)
    ap.add_argument("--observers", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast", "cast_perf.jsonl"))
    args = ap.parse_args()
    import torch
    from horayzon_amd import _lib
    n, off, A, E = args.tile, 16, args.azim, args.elev
    t, g, mask = terrain(n, off)
    dev = "cuda:%d" % t.device
    three = named_observers(g, n, off)
    obs = np.ascontiguousarray(np.vstack([three, lattice_observers(g, n, off, max(args.observers - 3, 0))])[:args.observers], np.float32)
    S = obs.shape[0]
    azim = np.linspace(0.0, 2.0 * np.pi, A, endpoint=False).astype(np.float32)
    elev = np.linspace(-np.pi / 2, np.pi / 2, E).astype(np.float32)
    max_dist = 5.0e4

    # (a) the panorama's rays, in image order [S][E][A]
    d_obs = torch.from_numpy(obs).to(dev)
    az, el = torch.from_numpy(azim).to(dev).double(), torch.from_numpy(elev).to(dev).double()
    image = torch.stack([(torch.cos(el)[:, None] * torch.sin(az)[None, :]), (torch.cos(el)[:, None] * torch.cos(az)[None, :]),
                         torch.sin(el)[:, None].expand(E, A)], dim=-1).float()
    d_dirs = image[None].expand(S, E, A, 3).reshape(-1, 3).contiguous()
    d_org = d_obs[:, None, :].expand(S, E * A, 3).reshape(-1, 3).contiguous()
    R = d_org.shape[0]
    del image, az, el
    # (b) the same rays in a random permutation
    perm = torch.randperm(R, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    s_org, s_dirs = d_org[perm].contiguous(), d_dirs[perm].contiguous()
    del perm
    # ... and in panorama's wave shape: tiles of 8 elevations x 8 azimuths, 64 consecutive rays each
    e_i = torch.arange(E, device=dev)[:, None].expand(E, A)
    a_i = torch.arange(A, device=dev)[None, :].expand(E, A)
    tile_key = (((e_i // 8) * ((A + 7) // 8) + a_i // 8) * 64 + (e_i % 8) * 8 + a_i % 8).reshape(-1)
    tiled = torch.argsort(tile_key)
    tiled = (torch.arange(S, device=dev)[:, None] * (E * A) + tiled[None, :]).reshape(-1)
    t_org, t_dirs = d_org[tiled].contiguous(), d_dirs[tiled].contiguous()
    del e_i, a_i, tile_key, tiled
    # (c) the viewshed's segments of the summit observer: target point of every inner cell (planar frames: 0.05 m up)
    in0 = in1 = n - 2 * off
    v = torch.from_numpy(np.ascontiguousarray(g["vert_grid"][:3 * n * n]).reshape(n, n, 3)[off:off + in0, off:off + in1].copy()).to(dev)
    seg_org = (v + torch.tensor([0.0, 0.0, 0.05], dtype=torch.float32, device=dev)).reshape(-1, 3).contiguous()
    seg_tgt = d_obs[0][None, :].expand(seg_org.shape[0], 3).contiguous()
    del v
    C = seg_org.shape[0]
    perm = torch.randperm(C, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    sseg_org, sseg_tgt = seg_org[perm].contiguous(), seg_tgt[perm].contiguous()
    del perm

    p_dist = torch.empty((S, E, A), dtype=torch.float32, device=dev)
    p_hits = torch.empty(S, dtype=torch.int64, device=dev)
    c_dist = torch.empty(R, dtype=torch.float32, device=dev)
    c_occ = torch.empty(R, dtype=torch.uint8, device=dev)
    codes = torch.empty((1, in0, in1), dtype=torch.uint8, device=dev)
    seg_occ = torch.empty(C, dtype=torch.uint8, device=dev)
    seg_dist = torch.empty(C, dtype=torch.float32, device=dev)
    h_org, h_dirs = d_org.cpu().numpy(), d_dirs.cpu().numpy()
    h_dist = np.empty(R, np.float32)
    torch.cuda.synchronize()
    print("%d rays, %d segments" % (R, C), file=sys.stderr, flush=True)

    def sort_only():
        _lib.check(_lib.lib().hz_debug_set(b"cast_sort_only", 1))
        try:
            t.cast(s_org, s_dirs, max_dist=max_dist, dist=c_dist, order="sorted")
        finally:
            _lib.check(_lib.lib().hz_debug_set(b"cast_sort_only", -1))

    # name -> (rays of the call, the call, where its hits are counted)
    passes = {
        "panorama": (R, lambda: t.panorama(d_obs, azim, elev, max_dist, dist=p_dist, hits=p_hits), lambda: int(p_hits.sum().item())),
        "cast_image": (R, lambda: t.cast(d_org, d_dirs, max_dist=max_dist, dist=c_dist), lambda: int((~torch.isnan(c_dist)).sum().item())),
        "cast_image_any": (R, lambda: t.cast(d_org, d_dirs, max_dist=max_dist, occluded=c_occ), lambda: int(c_occ.sum(dtype=torch.int64).item())),
        "cast_shuffled_given": (R, lambda: t.cast(s_org, s_dirs, max_dist=max_dist, dist=c_dist), lambda: int((~torch.isnan(c_dist)).sum().item())),
        "cast_shuffled_sorted": (R, lambda: t.cast(s_org, s_dirs, max_dist=max_dist, dist=c_dist, order="sorted"),
                                 lambda: int((~torch.isnan(c_dist)).sum().item())),
        "cast_shuffled_sort_only": (R, sort_only, None),
        "cast_image_sorted": (R, lambda: t.cast(d_org, d_dirs, max_dist=max_dist, dist=c_dist, order="sorted"),
                              lambda: int((~torch.isnan(c_dist)).sum().item())),
        "cast_image_tiled": (R, lambda: t.cast(t_org, t_dirs, max_dist=max_dist, dist=c_dist), lambda: int((~torch.isnan(c_dist)).sum().item())),
        "viewshed": (C, lambda: t.viewshed(d_obs[:1], visible=codes, facing=False), lambda: int((codes == 2).sum().item())),
        "cast_segments": (C, lambda: t.cast(seg_org, targets=seg_tgt, occluded=seg_occ), lambda: int(seg_occ.sum(dtype=torch.int64).item())),
        "cast_segments_dist": (C, lambda: t.cast(seg_org, targets=seg_tgt, occluded=seg_occ, dist=seg_dist),
                               lambda: int(seg_occ.sum(dtype=torch.int64).item())),
        "cast_segments_shuffled_given": (C, lambda: t.cast(sseg_org, targets=sseg_tgt, occluded=seg_occ),
                                         lambda: int(seg_occ.sum(dtype=torch.int64).item())),
        "cast_segments_shuffled_sorted": (C, lambda: t.cast(sseg_org, targets=sseg_tgt, occluded=seg_occ, order="sorted"),
                                          lambda: int(seg_occ.sum(dtype=torch.int64).item())),
        "cast_segments_dist_shuffled_given": (C, lambda: t.cast(sseg_org, targets=sseg_tgt, dist=seg_dist),
                                              lambda: int((~torch.isnan(seg_dist)).sum().item())),
        "cast_segments_dist_shuffled_sorted": (C, lambda: t.cast(sseg_org, targets=sseg_tgt, dist=seg_dist, order="sorted"),
                                               lambda: int((~torch.isnan(seg_dist)).sum().item())),
        "cast_image_numpy": (R, lambda: t.cast(h_org, h_dirs, max_dist=max_dist, dist=h_dist), lambda: int((~np.isnan(h_dist)).sum())),
    }
    kernel = {k: [] for k in passes}
    wall = {k: [] for k in passes}
    stats, hits = {}, {}
    for k, (_, fn, _) in passes.items():         # warm-up: code objects, staging buffers
        fn()
        print("warm-up %s: kernel %.3f ms" % (k, 1e3 * t.last_stats["t_kernel_s"]), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for k, (_, fn, count) in passes.items():
            t0 = time.perf_counter()
            fn()                                 # (every call ends in a stream synchronise of its own)
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
            kernel[k].append(t.last_stats["t_kernel_s"])
            stats[k] = dict(t.last_stats)
            hits[k] = None if count is None else count()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for k, (rays, _, _) in passes.items():
            med = statistics.median(kernel[k])
            d = {"pass": k, "tile": n, "azim_num": A, "elev_num": E, "observers": S, "repeats": args.repeats, "rays": rays,
                 "t_kernel_ms_median": round(1e3 * med, 3), "t_kernel_ms_min": round(1e3 * min(kernel[k]), 3),
                 "t_kernel_ms_max": round(1e3 * max(kernel[k]), 3), "ns_per_ray": round(1e9 * med / rays, 4),
                 "wall_ms_median": round(1e3 * statistics.median(wall[k]), 2), "num_rays": stats[k]["num_rays"],
                 "hit_share": None if hits[k] is None else round(hits[k] / rays, 4), "scratch_bytes": stats[k]["scratch_bytes"],
                 "bvh_height": stats[k]["bvh_height"]}
            print(json.dumps(d), flush=True)
            f.write(json.dumps(d) + "\n")
    # the words do not depend on the order or on where the arrays live
    t.cast(d_org, d_dirs, max_dist=max_dist, dist=c_dist)
    a = c_dist.view(torch.int32).clone()
    t.cast(d_org, d_dirs, max_dist=max_dist, dist=c_dist, order="sorted")
    torch.cuda.synchronize()
    print(json.dumps({"check": "image order: sorted == given", "equal": bool(torch.equal(a, c_dist.view(torch.int32))),
                      "numpy == hbm": bool(np.array_equal(h_dist.view(np.uint32), a.cpu().numpy().view(np.uint32)))}), flush=True)


if __name__ == "__main__":
    main()
