"""HorizonTerrain on the c3 tile (3601^2, 360 azimuths, the 144 sun positions of synth.sun_positions), everything resident in
HBM, against Terrain's ray casting of the same commit on the same box in the same run.

    python scripts/horisun_perf.py [--tile N] [--suns S] [--window W] [--layout both|cell_major|azim_major] [--refrac] [--out FILE]
    python scripts/horisun_perf.py --pmc [--layout cell_major|azim_major]   # only HorizonTerrain.sw_dir_cor_batch of one layout
        (k_horisun or k_horisun_planes), for a counter run of its own:
        rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -- python scripts/horisun_perf.py --pmc --layout azim_major

The tile's own horizon (guess_constant, dist_search 50 km, hori_acc 0.25 deg) is computed into a torch tensor in HBM and
borrowed by HorizonTerrain.  One warm-up and one timed pass of each call; one JSON line per figure:
  (a) sw_dir_cor_batch / shadow_batch / accumulate of HorizonTerrain and of Terrain, kernel ms per position (HIP events,
      last_stats) and wall ms; the float64 NumPy look-up on the host for a W x W window, ms per position, scaled by cells;
  (b) the bytes of horizon the batch must touch: the distinct 128-byte lines over all positions, counted from the float64
      look-up on the window and scaled to the tile (the achieved bytes come from the --pmc run: FETCH_SIZE of k_horisun,
      doubled as for every wide read on gfx950);
  (c) the share of unmasked (cell, position) pairs on which HorizonTerrain.shadow and Terrain.shadow agree -- a reported
      figure: the interpolated horizon is another model than a ray;
  (d) the azimuth-major layout (--layout both, the default; DESIGN.md section 4 clause 11), in the same run: the wall time of the
      horizon call into planes in HBM against the cell-major call, of to_azim_major on the tile's horizon, and (a) for a
      HorizonTerrain that reads the planes; the planes of the horizon call and of to_azim_major, and every output of the two
      layouts, are compared word for word on the whole tile;
  (e) --refrac: atmospheric refraction (DESIGN.md section 4 clause 13), in the same run: the rows of (a) again, marked
      "refrac": true, for HorizonTerrain with refraction(elevation) on in the layouts of the run and for Terrain(refrac_cor=True)
      as context, the outputs of the two layouts compared word for word on the whole tile, and the agreement of (c) for the
      refracted sun.
"""
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


def timed(fn, passes=1):
    """One warm-up, then `passes` timed passes: (result of the last pass, the median wall seconds)."""
    fn()
    walls = []
    for _ in range(passes):
        t0 = time.perf_counter()
        r = fn()
        walls.append(time.perf_counter() - t0)
    return r, sorted(walls)[len(walls) // 2]


def host_lookup(suns, hori, vert, vec_tilt, vec_norm, vec_north):
    """The look-up of DESIGN.md section 4 clause 10 in float64 NumPy on a window (set-up in float64 too: a speed and traffic
    yardstick, not the bit-exact reference of tests/horisun_reference.py).  Returns (shadow codes u8[S][y][x], the set of
    distinct (cell, 128-byte line of its row) pairs touched, as a count)."""
    A = hori.shape[2]
    n0, n1 = hori.shape[:2]
    o = vert.astype(np.float64) + 0.05 * vec_norm
    east = np.cross(vec_north.astype(np.float64), vec_norm.astype(np.float64))
    codes = np.empty((suns.shape[0], n0, n1), np.uint8)
    lines_per_row = (A * 4 + 127) // 128 + 1
    touched = np.zeros((n0, n1, lines_per_row), bool)
    row_byte0 = (np.arange(n0 * n1, dtype=np.int64).reshape(n0, n1) * A * 4) % 128      # offset of the row in its first line
    ii, jj = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    for s in range(suns.shape[0]):
        d = suns[s].astype(np.float64) - o
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        dot_ts = (vec_tilt * d).sum(axis=2)
        cn, ce, cu = (d * vec_north).sum(axis=2), (d * east).sum(axis=2), (d * vec_norm).sum(axis=2)
        phi = np.arctan2(ce, cn)
        phi[phi < 0.0] += 2.0 * np.pi
        u = phi * (A / (2.0 * np.pi))
        k = np.clip(np.floor(u), 0, A).astype(np.int64)
        t = u - k
        k0, k1 = k % A, (k + 1) % A
        h = (1.0 - t) * np.take_along_axis(hori, k0[..., None], 2)[..., 0] + t * np.take_along_axis(hori, k1[..., None], 2)[..., 0]
        shaded = np.arcsin(np.clip(cu, -1.0, 1.0)) < h
        faces = dot_ts > 0.0
        codes[s] = np.where(faces, np.where(shaded, 2, 0), 1)
        for kk in (k0, k1):
            line = (row_byte0 + kk * 4) // 128
            touched[ii[faces], jj[faces], line[faces]] = True
    return codes, int(touched.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--suns", type=int, default=144)
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--dist-search", type=float, default=50.0)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--layout", choices=("both", "cell_major", "azim_major"), default="both")
    ap.add_argument("--refrac", action="store_true", help="the speed rows again with atmospheric refraction on")
    ap.add_argument("--passes", type=int, default=3, help="timed passes of the layout figures (after one warm-up)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import horayzon_amd as hz
    from horayzon_amd import _lib, synth
    from horayzon_amd.shadow import gridded_azimuths
    n, off, A = args.tile, 16, args.azim
    g = synth.fractal_tile(n=n, offset=off)
    in0 = in1 = n - 2 * off
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

    # the tile's own horizon, written straight into HBM
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
    emit({"figure": "horizon", "tile": n, "azim_num": A, "t_kernel_ms": round(1e3 * st.t_kernel_s, 1),
          "hori_bytes": int(d_hori.numel()) * 4})

    planes = args.layout != "cell_major"
    d_planes = None
    if planes:
        # the same horizon as planes: by the horizon call itself and by the transposition of the cell-major result
        d_planes = torch.empty((A, in0, in1), dtype=torch.float32, device=dev)
        d_scratch = torch.empty((in0, in1, A), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        def horizon_call(layout):
            fn = L.hz_horizon_gridded_scene_planes if layout == "azim_major" else L.hz_horizon_gridded_scene_ex
            out = d_planes if layout == "azim_major" else d_scratch
            stc = _lib.hz_stats()
            _lib.check(fn(scene._h, _lib.ptr(vec_norm), _lib.ptr(vec_north), off, off, out.data_ptr(), in0, in1, A,
                          args.dist_search, 0.25, b"guess_constant", -15.0, d_mask.data_ptr(), 0.0, 0.01, C.byref(opts), None,
                          C.byref(stc)))
            return stc
        if not args.pmc:
            for layout in ("cell_major", "azim_major"):
                stc, wall = timed(lambda: horizon_call(layout), args.passes)
                emit({"figure": "horizon_step", "layout": layout, "tile": n, "azim_num": A, "wall_ms": round(1e3 * wall, 1),
                      "t_kernel_ms": round(1e3 * stc.t_kernel_s, 1), "scratch_bytes": int(stc.scratch_bytes)})
            same = bool(torch.equal(d_scratch.view(torch.int32), d_hori.view(torch.int32)))
            del d_scratch
            d_t, wall = timed(lambda: hz.horizon.to_azim_major(d_hori), args.passes)
            torch.cuda.synchronize()
            emit({"figure": "to_azim_major", "tile": n, "azim_num": A, "wall_ms": round(1e3 * wall, 1),
                  "gb_per_s_read_plus_written": round(2 * d_hori.numel() * 4 / wall / 1e9, 1),
                  "equal_to_the_horizon_calls_planes": bool(torch.equal(d_t.view(torch.int32), d_planes.view(torch.int32))),
                  "cell_major_calls_equal": same})
            del d_t
        else:
            del d_scratch
            _lib.check(L.hz_hori_to_planes(d_hori.data_ptr(), in0, in1, A, d_planes.data_ptr(), 0))

    th = hz.shadow.HorizonTerrain()
    th.initialise(gridded_azimuths(A), d_hori, g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, vec_north, enl, mask,
                  sw_dir_cor_fill=-7.0)
    th_p = None
    if planes:
        th_p = hz.shadow.HorizonTerrain()
        th_p.initialise_azim_major(gridded_azimuths(A), d_planes, g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, vec_north,
                                   enl, mask, sw_dir_cor_fill=-7.0)
    d_sw = torch.empty((S,) + shape, dtype=torch.float32, device=dev)
    if args.pmc:
        t_pmc = th_p if args.layout == "azim_major" else th
        timed(lambda: t_pmc.sw_dir_cor_batch(suns, d_sw))
        return
    tr = hz.shadow.Terrain()
    tr.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-7.0, scene=scene)
    d_sh = {"HorizonTerrain": torch.empty((S,) + shape, dtype=torch.uint8, device=dev),
            "Terrain": torch.empty((S,) + shape, dtype=torch.uint8, device=dev)}
    d_sum = torch.empty(shape, dtype=torch.float32, device=dev)
    d_lit = torch.empty(shape, dtype=torch.float32, device=dev)
    d_suns = torch.from_numpy(suns).to(dev)
    torch.cuda.synchronize()

    # (a) speed: the classes (and the two layouts of HorizonTerrain) alternate call by call
    classes = [("HorizonTerrain", "cell_major", th)] if args.layout != "azim_major" else []
    if planes:
        classes.append(("HorizonTerrain", "azim_major", th_p))
        d_sh["azim_major"] = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
        d_sw_p = torch.empty((S,) + shape, dtype=torch.float32, device=dev)
        d_sum_p, d_lit_p = torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)
    classes.append(("Terrain", None, tr))

    def speed(classes, refrac):
        for call in ("sw_dir_cor_batch", "shadow_batch", "accumulate"):
            for name, layout, t in classes:
                p = layout == "azim_major"
                if call == "sw_dir_cor_batch":
                    fn = lambda: t.sw_dir_cor_batch(suns, d_sw_p if p else d_sw)
                elif call == "shadow_batch":
                    fn = lambda: t.shadow_batch(suns, d_sh["azim_major" if p else name])
                else:
                    fn = lambda: t.accumulate(d_suns, None, sw_dir_cor_sum=d_sum_p if p else d_sum, sunlit_sum=d_lit_p if p else d_lit)
                _, wall = timed(fn, args.passes if layout else 1)
                torch.cuda.synchronize()
                d = {"figure": "speed", "class": name, "call": call, "tile": n, "suns": S,
                     "kernel_ms_per_position": round(1e3 * t.last_stats["t_kernel_s"] / S, 4),
                     "wall_ms_per_position": round(1e3 * wall / S, 4), "scratch_bytes": t.last_stats["scratch_bytes"]}
                if layout:
                    d["layout"] = layout
                if refrac:
                    d["refrac"] = True
                emit(d)
            if planes and args.layout == "both" and call != "accumulate":
                if call == "sw_dir_cor_batch":
                    # (Terrain's maps went to d_sw last: run the cell-major HorizonTerrain once more)
                    th.sw_dir_cor_batch(suns, d_sw)
                    torch.cuda.synchronize()
                a, b = (d_sw_p, d_sw) if call == "sw_dir_cor_batch" else (d_sh["azim_major"], d_sh["HorizonTerrain"])
                emit({"figure": "layouts_equal", "call": call, **({"refrac": True} if refrac else {}),
                      "equal": bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                b.view(torch.int32) if b.dtype == torch.float32 else b))})
        if planes and args.layout == "both":
            # (the sums of Terrain's accumulate went to d_sum / d_lit last: run the cell-major HorizonTerrain once more)
            th.accumulate(d_suns, None, sw_dir_cor_sum=d_sum, sunlit_sum=d_lit)
            torch.cuda.synchronize()
            emit({"figure": "layouts_equal", "call": "accumulate", **({"refrac": True} if refrac else {}),
                  "equal": bool(torch.equal(d_sum.view(torch.int32), d_sum_p.view(torch.int32))
                                and torch.equal(d_lit.view(torch.int32), d_lit_p.view(torch.int32)))})

    speed(classes, False)

    # (c) agreement of the look-up with ray casting on the tile's own horizon
    codes_h = d_sh["azim_major" if args.layout == "azim_major" else "HorizonTerrain"]
    same = 0
    for s in range(S):
        same += int((codes_h[s] == d_sh["Terrain"][s]).sum())
    emit({"figure": "agreement_with_ray_casting", "pairs": S * in0 * in1, "share_equal": round(same / (S * in0 * in1), 6)})

    # host look-up on a window (second comparison of (a)) and the lines it touches (b)
    W = min(args.window, in0)
    r0 = c0 = (in0 - W) // 2
    win = (slice(r0, r0 + W), slice(c0, c0 + W))
    hori_w = d_hori[r0:r0 + W, c0:c0 + W].cpu().numpy().astype(np.float64)
    verts = g["vert_grid"][:3 * n * n].reshape(n, n, 3)[off:off + in0, off:off + in1]
    t0 = time.perf_counter()
    codes_w, touched = host_lookup(suns, hori_w, verts[win], vec_tilt[win].astype(np.float64),
                                   vec_norm[win].astype(np.float64), vec_north[win].astype(np.float64))
    wall = time.perf_counter() - t0
    scale = (in0 * in1) / float(W * W)
    emit({"figure": "host_numpy_lookup", "window": W, "ms_per_position_window": round(1e3 * wall / S, 2),
          "ms_per_position_scaled_to_tile": round(1e3 * wall / S * scale, 1),
          "share_equal_to_gpu_codes": round(float((codes_w == codes_h[:, r0:r0 + W, c0:c0 + W].cpu().numpy()).mean()), 6)})
    emit({"figure": "horizon_lines", "window": W, "distinct_128B_lines_window": touched,
          "bytes_scaled_to_tile": int(touched * 128 * scale), "hori_bytes": int(d_hori.numel()) * 4,
          "output_bytes_sw_dir_cor_batch": S * in0 * in1 * 4})
    # (e) the same rows with atmospheric refraction
    if args.refrac:
        tr_r = hz.shadow.Terrain()
        tr_r.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-7.0,
                        refrac_cor=True, scene=scene)
        for _, _, t in classes[:-1]:
            t.refraction(elev)
        speed(classes[:-1] + [("Terrain", None, tr_r)], True)
        same = 0
        for s in range(S):
            same += int((codes_h[s] == d_sh["Terrain"][s]).sum())
        emit({"figure": "agreement_with_ray_casting", "refrac": True, "pairs": S * in0 * in1,
              "share_equal": round(same / (S * in0 * in1), 6)})
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
