"""The 16-bit horizon code (DESIGN.md section 4 clause 15) on the c3 tile (3601^2, 360 azimuths): what it costs and what it
saves, float32 and uint16 side by side in the same run.

    python scripts/q16_perf.py [--tile N] [--azim A] [--suns S] [--passes P] [--out FILE]

One warm-up, then the median of P = 3 timed passes of each call; one JSON line per figure (default FILE:
profiles/q16/q16_perf.jsonl):
  (a) "horizon_numpy": the NumPy-out horizon call on a prebuilt scene, hori_dtype float32 and uint16 in both layouts:
      wall seconds and the library's t_total_s, t_d2h_s, t_kernel_s, scratch_bytes.  (t_d2h_s: for float32 cell-major the
      chunk copies overlap the tracing and only the tail after the last chunk is counted; the float32 planes are copied
      inside the chunk loop and not counted; for uint16 the chunk copies are counted.  The wall time is the figure to compare.)
      "horizon_hbm": the same four calls with the output resident in HBM -- no copy, so the differences are the encoders.
  (b) "encoder": hz_hori_quantise / hz_hori_dequantise of the whole tile's horizon, HBM to HBM, against hz_debug_copy_peak.
  (c) "lookup": HorizonTerrain ms per position for shadow_batch and accumulate from codes and from float32, both layouts,
      without and with refraction; "lookup_equal": the outputs from codes against those of a float32 handle on
      dequantise(codes), word for word on the whole tile."""
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
    """One warm-up, then `passes` timed passes: (result of the last pass, median wall seconds, (min, max))."""
    fn()
    walls = []
    for _ in range(passes):
        t0 = time.perf_counter()
        r = fn()
        walls.append(time.perf_counter() - t0)
    return r, sorted(walls)[len(walls) // 2], (min(walls), max(walls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=3601)
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--suns", type=int, default=48)
    ap.add_argument("--dist-search", type=float, default=50.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--skip-numpy", action="store_true", help="leave out (a)'s NumPy-out calls (they need 2 x the horizon in host memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q16", "q16_perf.jsonl"))
    args = ap.parse_args()
    import torch
    import horayzon_amd as hz
    from horayzon_amd import _lib, synth
    from horayzon_amd.shadow import gridded_azimuths
    H = hz.horizon
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out_file = open(args.out, "w")

    def emit(d):
        d = dict(d, tile=n, azim_num=A)
        print(json.dumps(d), flush=True)
        out_file.write(json.dumps(d) + "\n")
        out_file.flush()

    L = _lib.lib()
    scene = hz.Scene.create(g["vert_grid"], n, n)
    kw = dict(vert_grid=g["vert_grid"], dem_dim_0=n, dem_dim_1=n, vec_norm=vec_norm, vec_north=vec_north, offset_0=off,
              offset_1=off, dist_search=args.dist_search, azim_num=A, mask=mask, scene=scene)
    combos = [(d, lay) for d in ("float32", "uint16") for lay in ("cell_major", "azim_major")]

    # (a) NumPy out
    if not args.skip_numpy:
        for dtype, layout in combos:
            def call():
                hori, _ = H.horizon_gridded(**kw, layout=layout, hori_dtype=dtype)
                return hori.nbytes, dict(H.last_stats)
            (nbytes, st), wall, spread = timed(call, args.passes)
            emit({"figure": "horizon_numpy", "hori_dtype": dtype, "layout": layout, "hori_bytes": nbytes,
                  "wall_s": round(wall, 3), "wall_min_max_s": [round(v, 3) for v in spread],
                  "t_total_s": round(st["t_total_s"], 3), "t_d2h_s": round(st["t_d2h_s"], 3),
                  "t_kernel_s": round(st["t_kernel_s"], 3), "scratch_bytes": int(st["scratch_bytes"])})

    # the same calls with the output in HBM; the buffers stay for (b) and (c)
    d_mask = torch.from_numpy(mask).to(dev)
    bufs = {("float32", "cell_major"): torch.empty((in0, in1, A), dtype=torch.float32, device=dev),
            ("float32", "azim_major"): torch.empty((A, in0, in1), dtype=torch.float32, device=dev),
            ("uint16", "cell_major"): torch.empty((in0, in1, A), dtype=torch.int16, device=dev),
            ("uint16", "azim_major"): torch.empty((A, in0, in1), dtype=torch.int16, device=dev)}
    torch.cuda.synchronize()
    opts = _lib.hz_opts()
    opts.device, opts.top_nodes, opts.regroup = 0, -1, -1

    def hbm_call(dtype, layout):
        st = _lib.hz_stats()
        planes = layout == "azim_major"
        head = (scene._h, _lib.ptr(vec_norm), _lib.ptr(vec_north), off, off, bufs[(dtype, layout)].data_ptr())
        tail = (in0, in1, A, args.dist_search, 0.25, b"guess_constant", -15.0, d_mask.data_ptr(), 0.0, 0.01, C.byref(opts), None,
                C.byref(st))
        if dtype == "uint16":
            _lib.check(L.hz_horizon_gridded_scene_q16(*head, int(planes), *tail))
        else:
            _lib.check((L.hz_horizon_gridded_scene_planes if planes else L.hz_horizon_gridded_scene_ex)(*head, *tail))
        return st
    for dtype, layout in combos:
        st, wall, spread = timed(lambda: hbm_call(dtype, layout), args.passes)
        emit({"figure": "horizon_hbm", "hori_dtype": dtype, "layout": layout, "wall_s": round(wall, 3),
              "wall_min_max_s": [round(v, 3) for v in spread], "t_kernel_s": round(st.t_kernel_s, 3),
              "scratch_bytes": int(st.scratch_bytes)})
    f_cell, f_planes = bufs[("float32", "cell_major")], bufs[("float32", "azim_major")]
    q_cell, q_planes = bufs[("uint16", "cell_major")], bufs[("uint16", "azim_major")]

    # (b) the elementwise encoder and decoder on the whole horizon, HBM to HBM
    n_el = f_cell.numel()
    d_q = torch.empty((in0, in1, A), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    _, wall_q, spread_q = timed(lambda: _lib.check(L.hz_hori_quantise(f_cell.data_ptr(), n_el, d_q.data_ptr(), 0)), args.passes)
    equal_q = bool(torch.equal(d_q, q_cell))
    equal_p = bool(torch.equal(H.quantise(f_planes).view(torch.int16), q_planes))
    gbs = C.c_double(0.0)
    _lib.check(L.hz_debug_copy_peak(0, 1 << 30, C.byref(gbs)))
    emit({"figure": "encoder", "kernel": "k_hori_quantise", "elements": n_el, "wall_ms": round(1e3 * wall_q, 2),
          "wall_min_max_ms": [round(1e3 * v, 2) for v in spread_q], "gb_per_s_read_plus_written": round(6 * n_el / wall_q / 1e9, 1),
          "copy_peak_gb_per_s": round(gbs.value, 1), "equal_to_the_horizon_calls_codes": equal_q,
          "planes_equal_to_the_horizon_calls_codes": equal_p})
    del d_q
    d_f = torch.empty((in0, in1, A), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _, wall_d, spread_d = timed(lambda: _lib.check(L.hz_hori_dequantise(q_cell.data_ptr(), n_el, d_f.data_ptr(), 0)), args.passes)
    err = float((d_f - f_cell).abs().max().item())
    emit({"figure": "encoder", "kernel": "k_hori_dequantise", "elements": n_el, "wall_ms": round(1e3 * wall_d, 2),
          "wall_min_max_ms": [round(1e3 * v, 2) for v in spread_d], "gb_per_s_read_plus_written": round(6 * n_el / wall_d / 1e9, 1),
          "copy_peak_gb_per_s": round(gbs.value, 1), "largest_error_rad": err, "bound_rad": H.Q16_MAX_ERROR})

    # (c) the look-up from codes and from float32
    azim = gridded_azimuths(A)
    common = (g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, vec_north, enl, mask)
    handles = []
    for dtype, layout in combos:
        t = hz.shadow.HorizonTerrain()
        if dtype == "uint16":
            t.initialise_q16(azim, bufs[(dtype, layout)], *common, sw_dir_cor_fill=-7.0, layout=layout)
        elif layout == "azim_major":
            t.initialise_azim_major(azim, f_planes, *common, sw_dir_cor_fill=-7.0)
        else:
            t.initialise(azim, f_cell, *common, sw_dir_cor_fill=-7.0)
        handles.append((dtype, layout, t))
    d_sh = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
    d_sum = torch.empty(shape, dtype=torch.float32, device=dev)
    d_lit = torch.empty(shape, dtype=torch.float32, device=dev)
    d_suns = torch.from_numpy(suns).to(dev)
    torch.cuda.synchronize()
    for refrac in (False, True):
        if refrac:
            for _, _, t in handles:
                t.refraction(elev)
        for call in ("shadow_batch", "accumulate"):
            for dtype, layout, t in handles:
                kernel = []

                def fn():
                    if call == "shadow_batch":
                        t.shadow_batch(suns, d_sh)
                    else:
                        t.accumulate(d_suns, None, sw_dir_cor_sum=d_sum, sunlit_sum=d_lit)
                    kernel.append(t.last_stats["t_kernel_s"])
                _, wall, spread = timed(fn, args.passes)
                k = sorted(kernel[1:])
                emit({"figure": "lookup", "call": call, "hori_dtype": dtype, "layout": layout, "refrac": refrac, "suns": S,
                      "kernel_ms_per_position": round(1e3 * k[len(k) // 2] / S, 4),
                      "kernel_ms_per_position_min_max": [round(1e3 * k[0] / S, 4), round(1e3 * k[-1] / S, 4)],
                      "wall_ms_per_position": round(1e3 * wall / S, 4)})
    # the contract on the whole tile: codes against a float32 handle on dequantise(codes) (refraction is on)
    del f_planes, bufs[("float32", "azim_major")]
    _lib.check(L.hz_hori_dequantise(q_cell.data_ptr(), n_el, d_f.data_ptr(), 0))
    td = hz.shadow.HorizonTerrain()
    td.initialise(azim, d_f, *common, sw_dir_cor_fill=-7.0)
    td.refraction(elev)
    d_sh2 = torch.empty((S,) + shape, dtype=torch.uint8, device=dev)
    d_sum2, d_lit2 = torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    td.shadow_batch(suns, d_sh2)
    td.accumulate(d_suns, None, sw_dir_cor_sum=d_sum2, sunlit_sum=d_lit2)
    for dtype, layout, t in handles:
        if dtype != "uint16":
            continue
        t.shadow_batch(suns, d_sh)
        t.accumulate(d_suns, None, sw_dir_cor_sum=d_sum, sunlit_sum=d_lit)
        torch.cuda.synchronize()
        emit({"figure": "lookup_equal", "layout": layout, "refrac": True,
              "equal": bool(torch.equal(d_sh, d_sh2) and torch.equal(d_sum.view(torch.int32), d_sum2.view(torch.int32))
                            and torch.equal(d_lit.view(torch.int32), d_lit2.view(torch.int32)))})
    # how often the quantisation moves a shadow code, against the float32 horizon (a reported figure)
    handles[0][2].shadow_batch(suns, d_sh2)
    torch.cuda.synchronize()
    moved = sum(int((d_sh[s] != d_sh2[s]).sum()) for s in range(S))
    emit({"figure": "codes_moved_by_quantisation", "refrac": True, "pairs": S * in0 * in1, "moved": moved})
    out_file.close()


if __name__ == "__main__":
    main()
