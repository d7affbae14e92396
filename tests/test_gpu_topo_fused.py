"""Sky view factor, visible sky fraction and topographic openness reduced from the horizon inside the horizon call
(horizon_gridded(topo=...), hz_horizon_gridded[_scene]_ex) and from a materialised horizon in one pass
(topo_param.topo_parameters, hz_topo_params).  Every fused map must be bit-identical to the single-output kernel on the
same horizon; the tiled kernel and its one-lane-per-cell fallback ("topo_wide") are checked alike."""
import contextlib
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

ALL = ("svf", "vsf", "openness")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svf_reference.npz")


class topo_wide:
    """hz_debug_set("topo_wide", 1) for the block, restored afterwards."""

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"topo_wide", 1))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"topo_wide", 0))
        return False


def _case(seed=31, n0=60, n1=72):
    g = cases.rough_terrain(n0, n1, seed=seed, offset=4, tilt_frames=True)
    kw = cases.grid_kwargs(g)
    tilt, *_ = cases.terrain_inputs(g)
    in0, in1 = kw["vec_norm"].shape[:2]
    mask = (np.random.default_rng(seed).random((in0, in1)) < 0.85).astype(np.uint8)
    mask[10:14, 20:30] = 0                             # a hole of masked cells
    return kw, tilt, dict(dist_search=2.0, elev_ang_low_lim=-40.0, mask=mask, hori_fill=-0.25)


def _separate(hip, azim, hori, tilt):
    T = hip.topo_param
    return {"svf": T.sky_view_factor(azim, hori, tilt), "vsf": T.visible_sky_fraction(azim, hori, tilt),
            "openness": T.topographic_openness(azim, hori)}


@pytest.mark.parametrize("azim_num", (36, 90))
def test_fused_equals_separate(hip, azim_num):
    kw, tilt, par = _case()
    for wide in (False, True):
        with topo_wide() if wide else contextlib.nullcontext():
            hori, azim, maps = hip.horizon.horizon_gridded(**kw, **par, azim_num=azim_num, topo=ALL, topo_vec_tilt=tilt)
            ref = _separate(hip, azim, hori, tilt)
        assert sorted(maps) == sorted(ALL)
        for name in ALL:
            assert maps[name].dtype == np.float32 and maps[name].shape == hori.shape[:2]
            assert not np.isnan(maps[name]).any(), name
            assert np.array_equal(maps[name], ref[name]), (name, wide)


def test_every_subset(hip):
    kw, tilt, par = _case(seed=32)
    par = dict(par, azim_num=36)
    hori, azim, full = hip.horizon.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=tilt)
    for k in (1, 2, 3):
        for sub in itertools.combinations(ALL, k):
            extra = dict(topo_vec_tilt=tilt) if ("svf" in sub or "vsf" in sub) else {}
            h, a, maps = hip.horizon.horizon_gridded(**kw, **par, topo=sub, **extra)
            assert np.array_equal(h, hori) and np.array_equal(a, azim)
            assert sorted(maps) == sorted(sub)
            for name in sub:
                assert np.array_equal(maps[name], full[name]), (sub, name)
    # "svf" alone is the old fused SVF path
    _, _, svf = hip.horizon.horizon_gridded(**kw, **par, svf_vec_tilt=tilt)
    _, _, maps = hip.horizon.horizon_gridded(**kw, **par, topo=("svf",), topo_vec_tilt=tilt)
    assert np.array_equal(maps["svf"], svf)
    # openness alone needs neither a tilt nor two azimuths
    h1, a1, m1 = hip.horizon.horizon_gridded(**kw, **dict(par, azim_num=1), topo=("openness",))
    assert list(m1) == ["openness"]
    assert np.array_equal(m1["openness"], hip.topo_param.topo_parameters(a1, h1, which=("openness",))["openness"])


@pytest.mark.parametrize("chunk", (0, 5, 16))
def test_topo_only(hip, chunk):
    kw, tilt, par = _case(seed=33)
    par = dict(par, azim_num=36)
    hori, azim, maps = hip.horizon.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=tilt)
    rays = hip.horizon.last_stats["num_rays"]
    none, a2, m2 = hip.horizon.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=tilt, topo_only=True, _chunk_rows=chunk)
    assert none is None and np.array_equal(a2, azim)
    assert hip.horizon.last_stats["num_rays"] == rays
    assert hip.horizon.last_stats["t_svf_s"] > 0.0
    for name in ALL:
        assert np.array_equal(m2[name], maps[name]), name
    # the same maps from row slabs stitched together, and from two threads on one device
    in0 = kw["vec_norm"].shape[0]
    stitched = {name: np.full(maps[name].shape, np.nan, np.float32) for name in ALL}
    for b, e in ((0, 9), (9, 30), (30, in0)):
        _, _, ms = hip.horizon.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=tilt, topo_only=True, rows=(b, e),
                                               _chunk_rows=chunk)
        for name in ALL:
            assert np.isnan(ms[name][:b]).all() and np.isnan(ms[name][e:]).all()
            stitched[name][b:e] = ms[name][b:e]
    _, _, md = hip.horizon.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=tilt, topo_only=True, devices=[0, 0],
                                           _chunk_rows=chunk)
    for name in ALL:
        assert np.array_equal(stitched[name], maps[name]), name
        assert np.array_equal(md[name], maps[name]), name


def test_device_resident_outputs(hip):
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    kw, tilt, par = _case(seed=34)
    A = 24
    hori, azim, maps = hip.horizon.horizon_gridded(**kw, **par, azim_num=A, topo=ALL, topo_vec_tilt=tilt)
    in0, in1 = hori.shape[:2]
    sc = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_norm = torch.from_numpy(kw["vec_norm"]).to(dev)
    d_north = torch.from_numpy(kw["vec_north"]).to(dev)
    d_mask = torch.from_numpy(par["mask"]).to(dev)
    d_tilt = torch.from_numpy(tilt).to(dev)

    def call(rb, re, slab):
        rows = re - rb
        n_out = rows if slab else in0
        d_hori = torch.full((n_out, in1, A), float("nan"), dtype=torch.float32, device=dev)
        d_svf, d_vsf, d_open = (torch.full((n_out, in1), float("nan"), dtype=torch.float32, device=dev) for _ in range(3))
        o = _lib.hz_opts()
        o.device = sc.device
        o.row_begin, o.row_end = rb, re
        o.hori_is_slab = int(slab)
        o.vec_tilt = d_tilt.data_ptr()
        o.svf = d_svf.data_ptr()
        t = _lib.hz_topo_out(d_vsf.data_ptr(), d_open.data_ptr())
        st = _lib.hz_stats()
        _lib.check(L.hz_horizon_gridded_scene_ex(sc._h, d_norm.data_ptr(), d_north.data_ptr(), kw["offset_0"], kw["offset_1"],
                                                 d_hori.data_ptr(), in0, in1, A, par["dist_search"], 0.25, b"guess_constant",
                                                 par["elev_ang_low_lim"], d_mask.data_ptr(), par["hori_fill"], 0.01,
                                                 C.byref(o), C.byref(t), C.byref(st)))
        torch.cuda.synchronize()
        return {"hori": d_hori.cpu().numpy(), "svf": d_svf.cpu().numpy(), "vsf": d_vsf.cpu().numpy(),
                "openness": d_open.cpu().numpy()}

    whole = call(0, in0, False)
    assert whole["hori"].tobytes() == hori.tobytes()
    for name in ALL:
        assert whole[name].tobytes() == maps[name].tobytes(), name
    rb, re = 11, 37
    slab = call(rb, re, True)
    assert slab["hori"].tobytes() == hori[rb:re].tobytes()
    for name in ALL:
        assert slab[name].tobytes() == maps[name][rb:re].tobytes(), name
    # a wrong hz_topo_out.size is rejected
    t = _lib.hz_topo_out()
    t.size = 4
    o = _lib.hz_opts()
    o.device = sc.device
    buf = np.empty((in0, in1, A), np.float32)
    rc = L.hz_horizon_gridded_scene_ex(sc._h, kw["vec_norm"].ctypes.data, kw["vec_north"].ctypes.data, kw["offset_0"],
                                       kw["offset_1"], buf.ctypes.data, in0, in1, A, 2.0, 0.25, b"guess_constant", -40.0,
                                       par["mask"].ctypes.data, 0.0, 0.01, C.byref(o), C.byref(t), None)
    assert rc == 1 and b"topo.size" in L.hz_last_error()
    sc.close()


def test_topo_parameters_on_reference_fixtures(hip):
    d = np.load(GOLDEN)
    T = hip.topo_param
    for n in "abc":
        azim, hori, tilt = d["azim_" + n], d["hori_" + n], d["tilt_" + n]
        for wide in (False, True):
            with topo_wide() if wide else contextlib.nullcontext():
                got = T.topo_parameters(azim, hori, tilt)
                ref = _separate(hip, azim, hori, tilt)
                pairs = {"svf": T.topo_parameters(azim, hori, tilt, which=("svf", "openness")),
                         "vsf": T.topo_parameters(azim, hori, tilt, which=("vsf", "openness"))}
            for name, key in (("svf", "svf_"), ("vsf", "vsf_"), ("openness", "top_")):
                assert np.abs(got[name] - d[key + n]).max() <= 1.0e-5, (n, name, wide)
                assert np.array_equal(got[name], ref[name]), (n, name, wide)
            for name, p in pairs.items():
                assert np.array_equal(p[name], ref[name]) and np.array_equal(p["openness"], ref["openness"]), (n, name)
        top_only = T.topo_parameters(azim, hori, which=("openness",))
        assert list(top_only) == ["openness"] and np.array_equal(top_only["openness"], T.topographic_openness(azim, hori))


def test_tile_band_topo_only(hip):
    """Rows 1800 - 1863 of the headline tile (3601^2, the 16-cell ring, 360 azimuths, 50 km): the maps of the call that
    never materialises the horizon equal topo_parameters on the materialised band."""
    from horayzon_amd import synth
    g = synth.fractal_tile()
    off, b, e = 16, 1800, 1864
    tilt, _ = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    kw = dict(vert_grid=g["vert_grid"], dem_dim_0=g["dem_dim_0"], dem_dim_1=g["dem_dim_1"],
              vec_norm=np.ascontiguousarray(g["vec_norm"][b:e]), vec_north=np.ascontiguousarray(g["vec_north"][b:e]),
              offset_0=off + b, offset_1=off)
    band_tilt = np.ascontiguousarray(tilt[b:e])
    sc = hip.Scene.create(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"])
    par = dict(dist_search=50.0, azim_num=360, elev_ang_low_lim=-15.0, scene=sc)
    none, azim, maps = hip.horizon.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=band_tilt, topo_only=True)
    assert none is None
    hori, azim2 = hip.horizon.horizon_gridded(**kw, **par)
    assert np.array_equal(azim, azim2)
    ref = hip.topo_param.topo_parameters(azim, hori, band_tilt)
    del hori
    for name in ALL:
        assert maps[name].shape == (e - b, 3569)
        assert np.array_equal(maps[name], ref[name]), name
    sc.close()
