"""Every way a gridded horizon leaves horizon_run (hz_api_horizon.hip): cell-major float32, planes, 16-bit codes and codes
as planes, into NumPy memory and into HBM, with and without the distances, in one chunk and in four (12 + 12 + 12 + 7 rows:
the double buffer of the streamed host output is reused twice), and a row slab with hori_is_slab both ways.  The inner domain
is 43 x 63 cells with 24 azimuths: an odd row length, odd plane strides, rows that are no multiple of 16.  One reference call
writes a cell-major float32 horizon into HBM in a single launch; every other call must give its words -- after
to_azim_major / quantise -- the words of the single-chunk cell-major distances, and the words of its three maps.  The
counts of hz_stats that do not depend on the launch schedule are the same in one chunk and in four, and scratch_bytes is what
the formulas of hz_horizon_plan.h (restated below) give."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

IN0, IN1, A, OFF = 43, 63, 24, 4
ROW_BYTES = IN1 * A * 4
DIST_SEARCH, HORI_ACC, LOW, FILL, ELEV = 2.0, 0.25, -15.0, -1.0, 0.01
KINDS = {"f32": 0, "planes": 1, "codes": 2, "codes_planes": 3}      # hori_kind: bit 0 planes, bit 1 16-bit codes
MAPS = ("svf", "vsf", "openness")
# hz_stats counts that one chunk and four chunks of the same call share: everything that is a property of the cells.  (As
# recorded before horizon_run was split up: 640145 rays, 699065 with the distances, 2455 cells, 3639 guard events in every
# case; left_cells is 1435 in one chunk and 1148 in four -- 8 x 8 blocks start at the chunk's first row -- and is not asserted)
SAME_IN_CHUNKS = ("num_rays", "num_cells", "guard_events", "rays_shortened", "near_used")
SENTINEL = 7.0


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(words(a), words(b))


@functools.lru_cache(maxsize=None)
def inputs():
    g = cases.rough_terrain(IN0 + 2 * OFF, IN1 + 2 * OFF, seed=19, offset=OFF)
    kw = cases.grid_kwargs(g)
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-0.4, 0.4, (IN0, IN1)), rng.uniform(-0.4, 0.4, (IN0, IN1))
    tilt = np.stack([np.sin(b), -np.sin(a) * np.cos(b), np.cos(a) * np.cos(b)], axis=2).astype(np.float32)
    mask = (rng.random((IN0, IN1)) >= 0.1).astype(np.uint8)
    return kw, tilt, mask


def call(hip, kind, dev, dist, chunk, rows=None, slab=False):
    """One call on a scene of its own (the scratch a scene keeps only grows).  Outputs in NumPy memory or (dev) in HBM,
    prefilled; returns the arrays as NumPy arrays and hz_stats as a dict."""
    import torch
    from horayzon_amd import _lib
    kw, tilt, mask = inputs()
    planes, q16 = bool(kind & 1), bool(kind & 2)
    rb, re = rows if rows else (0, IN0)
    n_out = re - rb if slab else IN0
    shape = (A, n_out, IN1) if planes else (n_out, IN1, A)
    tdev = torch.device("cuda:0")

    def buf(shp, dtype, fill):
        if dev:
            return torch.full(shp, fill, dtype={np.float32: torch.float32, np.uint16: torch.int16}[dtype], device=tdev)
        return np.full(shp, fill, dtype=dtype)

    hori = buf(shape, np.uint16 if q16 else np.float32, 0x1234 if q16 else SENTINEL)
    d = buf(shape, np.float32, SENTINEL) if dist else None
    maps = {n: buf((n_out, IN1), np.float32, SENTINEL) for n in MAPS}
    if dev:
        torch.cuda.synchronize()
    o = _lib.hz_opts()
    o.row_begin, o.row_end = (rb, re) if rows else (0, 0)
    o.hori_is_slab = int(slab)
    o.chunk_rows = chunk
    o.vec_tilt = _lib.ptr(tilt)
    o.svf = _lib.ptr(maps["svf"])
    t = _lib.hz_topo_out(_lib.ptr(maps["vsf"]), _lib.ptr(maps["openness"]))
    st = _lib.hz_stats()
    L = _lib.lib()
    sc = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])
    try:
        head = (sc._h, _lib.ptr(kw["vec_norm"]), _lib.ptr(kw["vec_north"]), kw["offset_0"], kw["offset_1"], _lib.ptr(hori))
        tail = (IN0, IN1, A, DIST_SEARCH, HORI_ACC, b"guess_constant", LOW, _lib.ptr(mask), FILL, ELEV,
                C.byref(o), C.byref(t), C.byref(st))
        if dist:
            rc = L.hz_horizon_gridded_scene_dist(*head, kind, _lib.ptr(d), *tail)
        elif q16:
            rc = L.hz_horizon_gridded_scene_q16(*head, int(planes), *tail)
        elif planes:
            rc = L.hz_horizon_gridded_scene_planes(*head, *tail)
        else:
            rc = L.hz_horizon_gridded_scene_ex(*head, *tail)
        _lib.check(rc)
    finally:
        sc.close()

    def host(a):
        if a is None or isinstance(a, np.ndarray):
            return a
        a = a.cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a
    if dev:
        torch.cuda.synchronize()
    out = {n: host(maps[n]) for n in MAPS}
    out.update(hori=host(hori), dist=host(d), stats=st.as_dict())
    return out


@functools.lru_cache(maxsize=None)
def reference(hip):
    """The cell-major float32 horizon and the three maps of one launch into HBM, and the cell-major distances of one chunk:
    computed once, shared, read only."""
    r = call(hip, 0, True, False, 0)
    rd = call(hip, 0, True, True, 0)
    assert same(rd["hori"], r["hori"])
    kw, tilt, mask = inputs()
    assert np.isfinite(r["hori"]).all() and (r["hori"][mask == 0] == np.float32(FILL)).all()
    assert np.isnan(rd["dist"][mask == 0]).all() and np.isfinite(rd["dist"][mask == 1]).any()
    ref = dict(r, dist=rd["dist"])
    for k in ("hori", "dist") + MAPS:
        ref[k].setflags(write=False)
    return ref


def laid_out(hip, a, kind):
    """`a` float32 (y, x, azim) as the call of `kind` returns it (the distances: without the code)."""
    if kind & 1:
        a = hip.horizon.to_azim_major(np.ascontiguousarray(a))
    return hip.horizon.quantise(a) if kind & 2 else a


# ---- hz_horizon_plan.h, restated -------------------------------------------------------------------------------------

def plan_chunk_rows(rows_all, row_bytes, target, fixed_rows):
    if fixed_rows > 0:
        return min(rows_all, fixed_rows)
    rows = max(16, min(rows_all, target // row_bytes))
    n_ch = (rows_all + rows - 1) // rows
    rows = min(rows, max(16, ((rows_all + n_ch - 1) // n_ch + 15) // 16 * 16))
    return min(rows, rows_all)


def plan_near_bytes(cells, azim_num):
    return ((cells * azim_num * 2 + 255) & ~255) + cells * 4


def tile_map_per_xcd(tiles_i, tiles_j):
    rj = max(1, (tiles_j + 7) // 8)
    pi = (tiles_i + rj - 1) // rj
    pi = min(max(pi, min(16, tiles_i // 4)), 64)
    pi = max(1, min(pi, tiles_i))
    ri = (tiles_i + pi - 1) // pi
    pi = (tiles_i + ri - 1) // ri
    return pi * ri * rj


def scan_temp_elems(n):
    total = 0
    while n > 2048:
        n = (n + 2047) // 2048
        total += n
    return total + 1


def sort_temp_elems(n):
    tiles = (n + 1023) // 1024
    return 2 * 256 * tiles + scan_temp_elems(256 * tiles)


def plan_left_bytes(rows_max, dim_in_1, thresholds=(36,)):
    units = tile_map_per_xcd((rows_max + 15) // 16, (dim_in_1 + 15) // 16) * 8 * 4
    total = cap_max = 0
    for t in thresholds:
        cap = ((units * t + 63) & ~63) + 64
        total += cap
        cap_max = max(cap_max, cap)
        units = cap // 64
    return total * 16 * 4 + (4 * cap_max + sort_temp_elems(cap_max) + 64) * 4


def expected_scratch(kind, dev, dist, chunk, rows=IN0):
    planes, q16 = bool(kind & 1), bool(kind & 2)
    direct = kind == 0 and dev                      # the kernels write a device hori_buffer in place: one launch
    cr = rows if direct else plan_chunk_rows(rows, ROW_BYTES, 4 << 30, chunk)
    tmp = 0 if direct else cr * ROW_BYTES
    if kind == 0 and not dev and cr < rows:
        tmp *= 2                                    # the second buffer of the streamed host output
    if kind == 1 and not dev:
        tmp *= 2                                    # the chunk as planes on its way to the host
    if q16 and not dev:
        tmp += cr * (ROW_BYTES // 2)                # the chunk as codes on its way to the host
    if dist and (not dev or planes):
        tmp += cr * ROW_BYTES                       # the chunk's cell-major distances
        if planes and not dev:
            tmp += cr * ROW_BYTES                   # ... and as planes on their way to the host
    return plan_near_bytes(cr * IN1, A) + plan_left_bytes(cr, IN1) + tmp


# ---- the tests ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dist", (False, True), ids=("hori", "hori+dist"))
@pytest.mark.parametrize("dev", (False, True), ids=("numpy", "hbm"))
@pytest.mark.parametrize("kind", sorted(KINDS), ids=sorted(KINDS))
def test_every_sink_in_one_chunk_and_in_four(hip, kind, dev, dist):
    pytest.importorskip("torch")
    k = KINDS[kind]
    ref = reference(hip)
    want_h = laid_out(hip, ref["hori"], k)
    want_d = laid_out(hip, ref["dist"], k & 1)
    runs = {}
    for chunk in (0, 12):
        r = runs[chunk] = call(hip, k, dev, dist, chunk)
        assert same(r["hori"], want_h), chunk
        if dist:
            assert same(r["dist"], want_d), chunk
        for n in MAPS:
            assert same(r[n], ref[n]), (n, chunk)
        st = r["stats"]
        print(kind, "hbm" if dev else "numpy", "dist" if dist else "", "chunk_rows", chunk,
              {n: st[n] for n in SAME_IN_CHUNKS + ("left_cells", "scratch_bytes")})
        assert st["near_used"] == 1 and st["height_field"] == 1
        assert st["scratch_bytes"] == expected_scratch(k, dev, dist, chunk), chunk
        mask = inputs()[2]
        assert st["num_cells"] == int(mask.sum())
        assert st["num_rays"] >= (2 if dist else 1) * int(mask.sum()) * A
    for n in SAME_IN_CHUNKS:
        assert runs[0]["stats"][n] == runs[12]["stats"][n], n


@pytest.mark.parametrize("dev", (False, True), ids=("numpy", "hbm"))
@pytest.mark.parametrize("kind", ("planes", "codes", "codes_planes"))
def test_row_slab_with_and_without_hori_is_slab(hip, kind, dev):
    """Rows 5 ... 37 in chunks of 12 (12 + 12 + 9), with the distances: the outputs hold the slab's rows only (hori_is_slab:
    a plane stride of 33 x 63 cells), or the whole domain, whose other rows stay as they were."""
    pytest.importorskip("torch")
    k = KINDS[kind]
    rb, re = 5, 38
    ref = reference(hip)
    rows = (lambda a: a[:, rb:re]) if k & 1 else (lambda a: a[rb:re])
    want_h = rows(laid_out(hip, ref["hori"], k))
    want_d = rows(laid_out(hip, ref["dist"], k & 1))
    mask = inputs()[2]
    for slab in (True, False):
        r = call(hip, k, dev, True, 12, rows=(rb, re), slab=slab)
        got_h, got_d = (r["hori"], r["dist"]) if slab else (rows(r["hori"]), rows(r["dist"]))
        assert same(np.ascontiguousarray(got_h), np.ascontiguousarray(want_h)), slab
        assert same(np.ascontiguousarray(got_d), np.ascontiguousarray(want_d)), slab
        for n in MAPS:
            assert same(np.ascontiguousarray(r[n] if slab else r[n][rb:re]), np.ascontiguousarray(ref[n][rb:re])), (n, slab)
        if not slab:                                # nothing outside the slab was written
            for a, fill in ((r["hori"], 0x1234 if k & 2 else SENTINEL), (r["dist"], SENTINEL)):
                rest = a.copy()
                rows(rest)[...] = fill
                assert (rest == fill).all()
            for n in MAPS:
                assert (r[n][:rb] == SENTINEL).all() and (r[n][re:] == SENTINEL).all(), n
        st = r["stats"]
        assert st["num_cells"] == int(mask[rb:re].sum())
        assert st["scratch_bytes"] == expected_scratch(k, dev, True, 12, rows=re - rb), slab
