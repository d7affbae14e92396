"""The horizon reductions on 16-bit codes and straight from planes (DESIGN.md section 4 clause 17), device-resident on the
3569^2 x 360 array of the headline tile: five routes side by side in the same run.

    python scripts/topo_q16_perf.py [--cells N] [--azim A] [--reps R] [--series S] [--out FILE]

Routes: "f32_cell" (k_topo, hz_topo_params), "q16_cell" (k_topo_q16), "f32_planes" (today's route of hz_topo_params_planes:
row slabs transposed back, then k_topo), "f32_planes_direct" (the same entry point under hz_debug_set("topo_planes_direct",
1): k_topo_planes<., float>) and "q16_planes" (k_topo_planes<., uint16_t>); outputs: "svf" alone and all three maps.
The horizon is synthetic (uniform in -30 ... 85 degrees) and is the DECODED code array on the float routes, so that all
five reduce the same numbers; "equal" says whether each route's maps are the words of f32_cell's.

Per (route, outputs): two warm-up calls, then R timed calls (wall clock around the library call, which ends with a
stream synchronisation; every array is in HBM, so no copy and no allocation is inside), reported as minimum and median;
the whole series is run S times and each series is a line of its own: the spread between series is the run-to-run spread.
One JSON line per figure (default FILE: profiles/topo_q16/topo_q16_perf.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROUTES = ("f32_cell", "q16_cell", "f32_planes", "f32_planes_direct", "q16_planes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=3569, help="the tile is cells x cells")
    ap.add_argument("--azim", type=int, default=360)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topo_q16", "topo_q16_perf.jsonl"))
    args = ap.parse_args()
    import torch
    import horayzon_amd as hz
    from horayzon_amd import _lib
    H = hz.horizon
    L = _lib.lib()
    n, A, dev = args.cells, args.azim, "cuda:0"
    ncell = n * n
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out_file = open(args.out, "w")

    def emit(d):
        d = dict(d, cells=[n, n], azim_num=A)
        print(json.dumps(d), flush=True)
        out_file.write(json.dumps(d) + "\n")
        out_file.flush()

    # the inputs, made on the device: codes of a seeded uniform horizon, their decoded float32, both as planes too
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    f_cell = torch.empty((n, n, A), dtype=torch.float32, device=dev)
    lo, hi = np.deg2rad(-30.0), np.deg2rad(85.0)
    for r0 in range(0, n, 256):
        f_cell[r0:r0 + 256].uniform_(lo, hi, generator=gen)
    q_cell = H.quantise(f_cell)
    f_cell = H.dequantise(q_cell)
    f_planes = H.to_azim_major(f_cell)
    q_planes = H.quantise(f_planes)
    slope = torch.empty((n, n), dtype=torch.float64, device=dev).uniform_(0.0, np.deg2rad(60.0), generator=gen)
    aspect = torch.empty((n, n), dtype=torch.float64, device=dev).uniform_(0.0, 2.0 * np.pi, generator=gen)
    d_tilt = torch.stack([slope.sin() * aspect.sin(), slope.sin() * aspect.cos(), slope.cos()], dim=-1).to(torch.float32).contiguous()
    del slope, aspect
    d_azim = torch.from_numpy(np.array([2.0 * np.pi / A * i for i in range(A)], np.float32)).to(dev)
    d_out = torch.empty((3, n, n), dtype=torch.float32, device=dev)
    d_ref = torch.empty((3, n, n), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    hori = {"f32_cell": f_cell, "q16_cell": q_cell, "f32_planes": f_planes, "f32_planes_direct": f_planes, "q16_planes": q_planes}
    bytes_read = {r: hori[r].numel() * hori[r].element_size() for r in ROUTES}

    def call(route, want, out):
        ptrs = [out[i].data_ptr() if w else None for i, w in enumerate(want)]
        tilt = d_tilt.data_ptr() if (want[0] or want[1]) else None
        h = hori[route].data_ptr()
        if route.startswith("q16"):
            rc = L.hz_topo_params_q16(d_azim.data_ptr(), h, int(route.endswith("planes")), tilt, n, n, A, *ptrs, 0)
        elif route == "f32_cell":
            rc = L.hz_topo_params(d_azim.data_ptr(), h, tilt, n, n, A, *ptrs, 0)
        else:
            _lib.check(L.hz_debug_set(b"topo_planes_direct", int(route == "f32_planes_direct")))
            try:
                rc = L.hz_topo_params_planes(d_azim.data_ptr(), h, tilt, n, n, A, *ptrs, 0)
            finally:
                _lib.check(L.hz_debug_set(b"topo_planes_direct", 0))
        _lib.check(rc)

    outputs = (("svf", (1, 0, 0)), ("svf+vsf+openness", (1, 1, 1)))
    # the contract on the whole tile: every route's maps against f32_cell's, as words
    call("f32_cell", (1, 1, 1), d_ref)
    for route in ROUTES[1:]:
        d_out.fill_(float("nan"))
        torch.cuda.synchronize()
        call(route, (1, 1, 1), d_out)
        torch.cuda.synchronize()
        emit({"figure": "equal", "route": route, "equal": bool(torch.equal(d_out.view(torch.int32), d_ref.view(torch.int32)))})
    for series in range(args.series):
        for name, want in outputs:
            for route in ROUTES:
                call(route, want, d_out)
                call(route, want, d_out)
                walls = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(route, want, d_out)
                    walls.append(time.perf_counter() - t0)
                walls.sort()
                med = walls[len(walls) // 2]
                emit({"figure": "reduce", "series": series, "route": route, "outputs": name, "reps": args.reps,
                      "ms_min": round(1e3 * walls[0], 3), "ms_median": round(1e3 * med, 3), "ms_max": round(1e3 * walls[-1], 3),
                      "hori_bytes": bytes_read[route], "gb_per_s_at_min": round(bytes_read[route] / walls[0] / 1e9, 1)})
    out_file.close()


if __name__ == "__main__":
    main()
