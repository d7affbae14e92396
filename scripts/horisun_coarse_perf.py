"""HorizonTerrain.sw_dir_cor_coarse on the c3 tile (3601^2, inner 3569^2, 360 azimuths, the 144 sun positions of
synth.sun_positions, 43 x 43 blocks), everything resident in HBM: the fused kernel against the two-pass route (the parent
commit's kernels) in the same process, for both horizon layouts.

    python scripts/horisun_coarse_perf.py [--tile N] [--suns S] [--pixels P] [--passes K] [--refrac] [--out FILE]

The tile's own horizon (guess_constant, dist_search 50 km, hori_acc 0.25 deg) is computed once into HBM, and
horizon.to_azim_major of it.  One warm-up, then the median of --passes timed passes of each call; one JSON line per row, with
the spread (max - min) of the passes.  Rows, per layout: fused with both outputs, fused with f_cor only, the two-pass route
(both outputs), and sw_dir_cor_batch + shadow_batch into HBM (the same information as maps, without the reduction); and
Terrain.sw_dir_cor_coarse (ray casting) on the same tile for context.  Untimed, word for word on the whole tile: fused
against two-pass, and planes against cell-major.  --refrac: every row and every comparison again, marked "refrac": true, with
refraction(elevation) on (DESIGN.md section 4 clause 13), and Terrain(refrac_cor=True).sw_dir_cor_coarse for context."""
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


def timed(fn, passes):
    """One warm-up, then `passes` timed passes: (median wall seconds, spread of the walls, median of fn's return values)."""
    fn()
    walls, rets = [], []
    for _ in range(passes):
        t0 = time.perf_counter()
        rets.append(fn())
        walls.append(time.perf_counter() - t0)
    return sorted(walls)[len(walls) // 2], max(walls) - min(walls), sorted(rets)[len(rets) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--suns", type=int, default=144)
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--pixels", type=int, default=43)
    ap.add_argument("--dist-search", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--refrac", action="store_true", help="the rows again with atmospheric refraction on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "horisun_coarse", "horisun_coarse_perf.jsonl"))
    args = ap.parse_args()
    import torch
    import horayzon_amd as hz
    from horayzon_amd import _lib, synth
    from horayzon_amd.shadow import gridded_azimuths
    n, off, A, P = args.tile, 16, args.azim, args.pixels
    g = synth.fractal_tile(n=n, offset=off)
    in0 = in1 = n - 2 * off
    assert in0 % P == 0, "--pixels must divide the inner domain"
    vec_tilt, enl = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    vec_norm, vec_north = synth.planar_frames(in0, in1)
    elev = np.ascontiguousarray(g["z"][off:off + in0, off:off + in1], np.float32)
    mask = np.ones((in0, in1), np.uint8)
    suns, _, _ = synth.sun_positions(num=args.suns)
    S = suns.shape[0]
    shape = mask.shape
    dev = "cuda:0"
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    L = _lib.lib()

    def knob(key, v):
        _lib.check(L.hz_debug_set(key, v))

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
    d_planes = hz.horizon.to_azim_major(d_hori)
    torch.cuda.synchronize()
    emit({"figure": "horizon", "tile": n, "azim_num": A, "t_kernel_ms": round(1e3 * st.t_kernel_s, 1),
          "hori_bytes": int(d_hori.numel()) * 4})

    objs = {}
    objs["cell_major"] = hz.shadow.HorizonTerrain()
    objs["cell_major"].initialise(gridded_azimuths(A), d_hori, g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, vec_north,
                                  enl, mask, sw_dir_cor_fill=-7.0)
    objs["azim_major"] = hz.shadow.HorizonTerrain()
    objs["azim_major"].initialise_azim_major(gridded_azimuths(A), d_planes, g["vert_grid"], n, n, off, off, vec_tilt, vec_norm,
                                             vec_north, enl, mask, sw_dir_cor_fill=-7.0)
    gy, gx = in0 // P, in1 // P
    d_suns = torch.from_numpy(suns).to(dev)

    def table():
        return torch.empty((S, gy, gx), dtype=torch.float32, device=dev)
    tables = {}
    d_sw = torch.empty((S,) + shape, dtype=torch.float32, device=dev)
    d_sh = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pairs = float(S) * in0 * in1

    def row(name, layout, t, fn, extra=None):
        def run():
            fn()
            torch.cuda.synchronize()
            return t.last_stats["t_kernel_s"]
        wall, spread, kern = timed(run, args.passes)
        d = {"figure": "speed", "row": name, "tile": n, "suns": S, "pixel_per_gc": P, "passes": args.passes,
             "wall_ms": round(1e3 * wall, 2), "wall_spread_ms": round(1e3 * spread, 2),
             "kernel_ms_last_call": round(1e3 * kern, 2), "wall_ns_per_pair": round(1e9 * wall / pairs, 4),
             "scratch_bytes": int(t.last_stats["scratch_bytes"])}
        if layout:
            d["layout"] = layout
        d.update(extra or {})
        emit(d)
        return wall, spread

    def measure(tag):
        walls = {}
        for layout, t in objs.items():
            f0, l0, f1, f2, l2 = table(), table(), table(), table(), table()
            tables[layout] = (f0, l0, f1, f2, l2)
            knob(b"horisun_coarse_route", 0)
            walls[(layout, "fused")] = row("fused", layout, t, lambda: t.sw_dir_cor_coarse(d_suns, P, f_cor=f0, sunlit_frac=l0), tag)
            row("fused_f_cor_only", layout, t, lambda: t.sw_dir_cor_coarse(d_suns, P, f_cor=f1), tag)
            knob(b"horisun_coarse_route", 1)
            walls[(layout, "two_pass")] = row("two_pass", layout, t, lambda: t.sw_dir_cor_coarse(d_suns, P, f_cor=f2, sunlit_frac=l2), tag)
            knob(b"horisun_coarse_route", -1)

            def maps():
                t.sw_dir_cor_batch(suns, d_sw)
                k = t.last_stats["t_kernel_s"]
                t.shadow_batch(suns, d_sh)
                t.last_stats["t_kernel_s"] += k
            row("batch_maps_into_hbm", layout, t, maps, {"map_bytes": int(d_sw.numel()) * 4 + int(d_sh.numel()), **tag})

        def words(a, b):
            return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        for layout in objs:
            f0, l0, f1, f2, l2 = tables[layout]
            emit({"figure": "equal", "what": "fused against two_pass", "layout": layout, **tag,
                  "f_cor": words(f0, f2), "sunlit_frac": words(l0, l2), "f_cor_only": words(f1, f0)})
        a, b = tables["cell_major"], tables["azim_major"]
        emit({"figure": "equal", "what": "azim_major against cell_major", **tag, "f_cor": words(a[0], b[0]), "sunlit_frac": words(a[1], b[1])})
        for layout in objs:
            (wf, sf), (wt, s2) = walls[(layout, "fused")], walls[(layout, "two_pass")]
            emit({"figure": "verdict", "layout": layout, **tag, "fused_wall_ms": round(1e3 * wf, 2), "two_pass_wall_ms": round(1e3 * wt, 2),
                  "margin_ms": round(1e3 * max(sf, s2), 2), "fused_is_not_slower": bool(wf <= wt + max(sf, s2))})

    measure({})
    if args.refrac:
        for t in objs.values():
            t.refraction(elev)
        measure({"refrac": True})

    # context: ray casting, the same tile and blocks
    del d_sw, d_sh
    tr = hz.shadow.Terrain()
    tr.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-7.0, scene=scene)
    fr, lr = table(), table()
    row("Terrain.sw_dir_cor_coarse", None, tr, lambda: tr.sw_dir_cor_coarse(d_suns, P, f_cor=fr, sunlit_frac=lr))
    if args.refrac:
        tr.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-7.0, refrac_cor=True,
                      scene=scene)
        row("Terrain.sw_dir_cor_coarse", None, tr, lambda: tr.sw_dir_cor_coarse(d_suns, P, f_cor=fr, sunlit_frac=lr),
            {"refrac": True})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
