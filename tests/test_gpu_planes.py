"""The azimuth-major horizon layout planes[azim][y][x] (DESIGN.md section 4 clause 11; hz_planes.hip): the transpositions,
horizon_gridded(layout="azim_major"), HorizonTerrain.initialise_azim_major and the topo_param reductions on planes.

The contract is that planes[k][y][x] and hori[y][x][k] hold the same 32-bit word and that nothing numerical is decided
anew, so every comparison here is exact: on the uint32 view wherever a NaN can occur."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from horayzon_amd.shadow import gridded_azimuths
from tests import cases
from tests import horisun_reference as R

pytestmark = pytest.mark.gpu

ALL = ("svf", "vsf", "openness")
# cells and azimuths just below, on and just above the edges of the 64-cell x 32-azimuth tile
SHAPES = [(1, 1, 1), (3, 5, 2), (1, 63, 31), (1, 64, 32), (5, 13, 33), (1, 129, 64), (7, 67, 65), (16, 130, 360)]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(words(a), words(b))


class knob:
    """hz_debug_set(key, value) for the block, the default restored afterwards."""

    def __init__(self, key, value, default):
        self.key, self.value, self.default = key, value, default

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.default))
        return False


def random_words(shape, seed):
    """Random 32-bit patterns viewed as float32: NaNs with payloads, infinities and denormals occur."""
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32).view(np.float32)


# ---- 1. transposition -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transposition_host_and_device(hip, shape):
    torch = pytest.importorskip("torch")
    H = hip.horizon
    h = random_words(shape, seed=sum(shape))
    want = np.ascontiguousarray(np.transpose(h, (2, 0, 1)))
    if h.size >= 10000:
        assert np.isnan(h).any()                                  # (1 pattern in 256 is a NaN, payloads of all kinds)
    p = H.to_azim_major(h)
    assert isinstance(p, np.ndarray) and same_words(p, want)
    back = H.to_cell_major(p)
    assert isinstance(back, np.ndarray) and same_words(back, h)
    # staged in several chunks (host sides): 100 cells per chunk, no multiple of the tile
    with knob(b"planes_chunk", 100, -1):
        assert same_words(H.to_azim_major(h), want) and same_words(H.to_cell_major(want), h)
    # device tensors in, device tensors out, the same words (compared as int32: no float compare touches a NaN)
    d_h = torch.from_numpy(h.view(np.int32)).to("cuda:0").view(torch.float32)
    torch.cuda.synchronize()
    d_p = H.to_azim_major(d_h)
    assert isinstance(d_p, torch.Tensor) and d_p.is_cuda and tuple(d_p.shape) == want.shape
    torch.cuda.synchronize()
    assert np.array_equal(d_p.view(torch.int32).cpu().numpy().view(np.uint32), words(want))
    d_back = H.to_cell_major(d_p)
    torch.cuda.synchronize()
    assert np.array_equal(d_back.view(torch.int32).cpu().numpy().view(np.uint32), words(h))


def test_transposition_mixed_sides_through_the_c_abi(hip):
    """One side host, one side device, both directions, in several staging chunks."""
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    L = _lib.lib()
    shape = (7, 67, 65)
    h = random_words(shape, seed=5)
    want = np.ascontiguousarray(np.transpose(h, (2, 0, 1)))
    d_h = torch.from_numpy(h.view(np.int32)).to("cuda:0")
    d_want = torch.from_numpy(want.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    with knob(b"planes_chunk", 130, -1):
        p = np.zeros(want.shape, np.float32)
        _lib.check(L.hz_hori_to_planes(d_h.data_ptr(), *shape, p.ctypes.data, 0))
        assert same_words(p, want)
        d_p = torch.zeros(want.shape, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        _lib.check(L.hz_hori_to_planes(h.ctypes.data, *shape, d_p.data_ptr(), 0))
        assert np.array_equal(d_p.cpu().numpy().view(np.uint32), words(want))
        b = np.zeros(shape, np.float32)
        _lib.check(L.hz_hori_from_planes(d_want.data_ptr(), *shape, b.ctypes.data, 0))
        assert same_words(b, h)
        d_b = torch.zeros(shape, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        _lib.check(L.hz_hori_from_planes(want.ctypes.data, *shape, d_b.data_ptr(), 0))
        assert np.array_equal(d_b.cpu().numpy().view(np.uint32), words(h))


# ---- 2. the horizon call ----------------------------------------------------------------------------------------

_HORIZON = {}


def horizon_case():
    """Inputs of the horizon tests, built once and left unchanged: a 60 x 72 DEM, inner domain 52 x 64, a mask with holes."""
    if not _HORIZON:
        g = cases.rough_terrain(60, 72, seed=31, offset=4, tilt_frames=True)
        kw = cases.grid_kwargs(g)
        tilt, *_ = cases.terrain_inputs(g)
        in0, in1 = kw["vec_norm"].shape[:2]
        mask = (np.random.default_rng(31).random((in0, in1)) < 0.85).astype(np.uint8)
        mask[10:14, 20:30] = 0
        _HORIZON.update(kw=kw, tilt=tilt, par=dict(dist_search=2.0, elev_ang_low_lim=-40.0, mask=mask, hori_fill=np.nan))
    return _HORIZON["kw"], _HORIZON["tilt"], _HORIZON["par"]


@pytest.mark.parametrize("alg", ("guess_constant", "binary_search"))
@pytest.mark.parametrize("azim_num", (36, 5))
def test_horizon_call_writes_the_transpose(hip, alg, azim_num):
    kw, tilt, par = horizon_case()
    H = hip.horizon
    in0 = kw["vec_norm"].shape[0]
    chunk = 20                                                    # 52 rows: chunks of 20, 20 and 12
    hori, azim, maps = H.horizon_gridded(**kw, **par, azim_num=azim_num, ray_algorithm=alg, topo=ALL, topo_vec_tilt=tilt)
    st_cell = dict(H.last_stats)
    assert np.isnan(hori).any()                                   # masked cells: hori_fill = NaN
    want = np.ascontiguousarray(np.transpose(hori, (2, 0, 1)))
    planes, azim_p, maps_p = H.horizon_gridded(**kw, **par, azim_num=azim_num, ray_algorithm=alg, topo=ALL, topo_vec_tilt=tilt,
                                               layout="azim_major", _chunk_rows=chunk)
    st = dict(H.last_stats)
    assert planes.dtype == np.float32 and planes.shape == (azim_num, in0, hori.shape[1])
    assert same_words(planes, want) and np.array_equal(azim_p, azim)
    for name in ALL:
        assert same_words(maps_p[name], maps[name]), name
    assert st["num_rays"] == st_cell["num_rays"] and st["num_cells"] == st_cell["num_cells"]
    assert st["scratch_bytes"] >= 2 * chunk * hori.shape[1] * azim_num * 4      # both chunk buffers are counted
    # without topo, in one chunk, and with the sky view factor of svf_vec_tilt
    plain, _ = H.horizon_gridded(**kw, **par, azim_num=azim_num, ray_algorithm=alg, layout="azim_major")
    assert same_words(plain, want)
    if azim_num >= 2:
        with_svf, _, svf = H.horizon_gridded(**kw, **par, azim_num=azim_num, ray_algorithm=alg, svf_vec_tilt=tilt,
                                             layout="azim_major", _chunk_rows=chunk)
        assert same_words(with_svf, want) and same_words(svf, maps["svf"])


def test_horizon_call_rows_scene_and_devices(hip):
    kw, tilt, par = horizon_case()
    H = hip.horizon
    A = 36
    hori, _ = H.horizon_gridded(**kw, **par, azim_num=A)
    want = np.ascontiguousarray(np.transpose(hori, (2, 0, 1)))
    in0 = hori.shape[0]
    b, e = 9, 41                                                  # strictly inside; 32 rows in chunks of 12, 12 and 8
    part, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout="azim_major", rows=(b, e), _chunk_rows=12)
    assert same_words(part[:, b:e], want[:, b:e])
    assert np.isnan(part[:, :b]).all() and np.isnan(part[:, e:]).all()          # the other rows of every plane
    sc = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])
    on_scene, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout="azim_major", scene=sc, _chunk_rows=20)
    sc.close()
    assert same_words(on_scene, want)
    one, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout="azim_major", devices=[0])
    two, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout="azim_major", devices=[0, 0], _chunk_rows=7)
    assert same_words(one, want) and same_words(two, want)
    assert in0 == 52


def test_horizon_call_device_resident_planes(hip):
    """hz_horizon_gridded_scene_planes with hori_planes in HBM: the whole domain, and a slab with hori_is_slab."""
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    kw, tilt, par = horizon_case()
    A = 24
    hori, azim, maps = hip.horizon.horizon_gridded(**kw, **par, azim_num=A, topo=ALL, topo_vec_tilt=tilt)
    want = np.ascontiguousarray(np.transpose(hori, (2, 0, 1)))
    in0, in1 = hori.shape[:2]
    sc = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_norm = torch.from_numpy(kw["vec_norm"]).to(dev)
    d_north = torch.from_numpy(kw["vec_north"]).to(dev)
    d_mask = torch.from_numpy(par["mask"]).to(dev)
    d_tilt = torch.from_numpy(tilt).to(dev)

    def call(rb, re, slab, chunk):
        n_out = re - rb if slab else in0
        d_planes = torch.full((A, n_out, in1), 7.0, dtype=torch.float32, device=dev)
        d_svf, d_vsf, d_open = (torch.full((n_out, in1), 7.0, dtype=torch.float32, device=dev) for _ in range(3))
        torch.cuda.synchronize()
        o = _lib.hz_opts()
        o.device = sc.device
        o.row_begin, o.row_end = rb, re
        o.hori_is_slab = int(slab)
        o.chunk_rows = chunk
        o.vec_tilt = d_tilt.data_ptr()
        o.svf = d_svf.data_ptr()
        t = _lib.hz_topo_out(d_vsf.data_ptr(), d_open.data_ptr())
        st = _lib.hz_stats()
        _lib.check(L.hz_horizon_gridded_scene_planes(sc._h, d_norm.data_ptr(), d_north.data_ptr(), kw["offset_0"],
                                                     kw["offset_1"], d_planes.data_ptr(), in0, in1, A, par["dist_search"], 0.25,
                                                     b"guess_constant", par["elev_ang_low_lim"], d_mask.data_ptr(),
                                                     par["hori_fill"], 0.01, C.byref(o), C.byref(t), C.byref(st)))
        torch.cuda.synchronize()
        return {"planes": d_planes.cpu().numpy(), "svf": d_svf.cpu().numpy(), "vsf": d_vsf.cpu().numpy(),
                "openness": d_open.cpu().numpy()}

    whole = call(0, in0, False, 20)
    assert same_words(whole["planes"], want)
    for name in ALL:
        assert same_words(whole[name], maps[name]), name
    rb, re = 11, 37
    slab = call(rb, re, True, 10)                                 # the planes hold the slab's rows only: stride 26 rows
    assert same_words(slab["planes"], np.ascontiguousarray(want[:, rb:re]))
    for name in ALL:
        assert same_words(slab[name], np.ascontiguousarray(maps[name][rb:re])), name
    inside = call(rb, re, False, 10)                              # whole-domain planes, rows outside the slab untouched
    assert same_words(np.ascontiguousarray(inside["planes"][:, rb:re]), np.ascontiguousarray(want[:, rb:re]))
    assert (inside["planes"][:, :rb] == 7.0).all() and (inside["planes"][:, re:] == 7.0).all()
    sc.close()


# ---- 3. HorizonTerrain ------------------------------------------------------------------------------------------

_TERRAIN = {}


def terrain_case(azim_num):
    """37 x 53 cells (no multiple of the workgroup's 256), per-cell random frames (A = 1, 2: the lanes of a wave ask for
    different planes) or the planar frame (A = 5, 36), masked cells, ang_max = 85 so that grazing suns fall beyond it; 8
    positions, among them (R.make_case) the zenith, a sun a hair west of north -- the last sector, k1 wraps to plane 0 -- and
    one exactly north, plus one 14 degrees below the horizontal: below every horizon (>= -0.2 rad) in the planar frame."""
    if azim_num not in _TERRAIN:
        c = R.make_case((37, 53), (45, 61), (4, 4), azim_num, 8, "planar" if azim_num in (5, 36) else "random", 300 + azim_num,
                        ang_max=85.0)
        c["planar"] = azim_num in (5, 36)
        centre = c["vert"][18, 26].astype(np.float64)
        low = np.deg2rad(-14.0)
        c["suns"][0] = (centre + 1.5e11 * np.array([np.cos(low) * 0.6, np.cos(low) * 0.8, np.sin(low)])).astype(np.float32)
        c["planes"] = np.ascontiguousarray(np.transpose(c["hori"], (2, 0, 1)))
        _TERRAIN[azim_num] = c
    return _TERRAIN[azim_num]


def make_terrain(hip, c, hori, planes):
    t = hip.shadow.HorizonTerrain()
    init = t.initialise_azim_major if planes else t.initialise
    init(gridded_azimuths(c["azim_num"]), hori, c["vert_grid"], c["dem_dim_0"], c["dem_dim_1"], c["offset_0"], c["offset_1"],
         c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], c["mask"], sw_dir_cor_fill=c["fill"],
         ang_max=c["ang_max"])
    return t


def all_outputs(t, c, w):
    suns, shape = c["suns"], c["mask"].shape
    S = suns.shape[0]
    out = dict(one_sh=np.full(shape, 77, np.uint8), one_sw=np.full(shape, 77.0, np.float32),
               sh=np.full((S,) + shape, 77, np.uint8), sw=np.full((S,) + shape, 77.0, np.float32),
               a_sh=np.full((S,) + shape, 77, np.uint8), a_sw=np.full((S,) + shape, 77.0, np.float32),
               sum_sw=np.full(shape, 77.0, np.float32), sum_lit=np.full(shape, 77.0, np.float32))
    t.shadow(suns[S - 2], out["one_sh"])
    t.sw_dir_cor(suns[S - 2], out["one_sw"])
    t.shadow_batch(suns, out["sh"])
    t.sw_dir_cor_batch(suns, out["sw"])
    t.accumulate(suns, w, sw_dir_cor_sum=out["sum_sw"], sunlit_sum=out["sum_lit"], shadow_buffers=out["a_sh"],
                 sw_dir_cor_buffers=out["a_sw"])
    return out


@pytest.mark.parametrize("azim_num", (1, 2, 5, 36))
def test_horizon_terrain_reads_planes(hip, azim_num):
    torch = pytest.importorskip("torch")
    c = terrain_case(azim_num)
    S = c["suns"].shape[0]
    w = np.random.default_rng(9).uniform(0.05, 3.0, S).astype(np.float32)
    w[::4] = 0.0
    with knob(b"horisun_chunk", 3, -1):                           # 8 positions: launches of 3, 3 and 2
        ref = all_outputs(make_terrain(hip, c, c["hori"], False), c, w)
        got = all_outputs(make_terrain(hip, c, c["planes"], True), c, w)
        d_planes = torch.from_numpy(c["planes"]).to("cuda:0")
        torch.cuda.synchronize()
        td = make_terrain(hip, c, d_planes, True)
        assert td._hori is d_planes                               # borrowed: the object holds a reference
        got_dev = all_outputs(td, c, w)
    one = all_outputs(make_terrain(hip, c, c["planes"], True), c, w)           # the default chunk: one launch
    for name, a in ref.items():
        assert a.tobytes() == got[name].tobytes(), name
        assert a.tobytes() == got_dev[name].tobytes(), name
        assert a.tobytes() == one[name].tobytes(), name
    # the cases this test is about did occur
    sh, sw, mask = ref["sh"], ref["sw"], c["mask"]
    assert (mask != 1).any() and (sh[:, mask != 1] == 3).all()
    for code in (0, 1, 2):
        assert (sh == code).any(), code
    if c["planar"]:
        assert not (sh[0][mask == 1] == 0).any() and (sh[0] == 2).any()      # the sun below every horizon lights nothing
    assert ((sh == 0) & (sw == 0.0)).any()                        # lit, but beyond ang_max
    assert np.array_equal(ref["one_sh"], sh[S - 2])               # the sun in the last sector (k1 = plane 0)


# ---- 4. topo_param on planes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("azim_num", (2, 36))
def test_topo_param_on_planes(hip, azim_num):
    T = hip.topo_param
    rng = np.random.default_rng(40 + azim_num)
    shape = (45, 67)
    hori = rng.uniform(-0.3, 1.2, shape + (azim_num,)).astype(np.float32)
    hori[3, 5] = np.nan
    n = rng.standard_normal(shape + (3,))
    n[..., 2] = np.abs(n[..., 2]) + 0.3
    tilt = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    azim = gridded_azimuths(azim_num)
    planes = np.ascontiguousarray(np.transpose(hori, (2, 0, 1)))
    for wide in (False, True):
        with knob(b"topo_wide", 1, 0) if wide else contextlib.nullcontext():
            ref = {"svf": T.sky_view_factor(azim, hori, tilt), "vsf": T.visible_sky_fraction(azim, hori, tilt),
                   "openness": T.topographic_openness(azim, hori)}
            ref_all = T.topo_parameters(azim, hori, tilt)
            for chunk in (-1, 200):                               # one chunk; chunks of 2 rows (200 // 67) with a ragged last one
                with knob(b"planes_chunk", chunk, -1):
                    got = {"svf": T.sky_view_factor(azim, planes, tilt, layout="azim_major"),
                           "vsf": T.visible_sky_fraction(azim, planes, tilt, layout="azim_major"),
                           "openness": T.topographic_openness(azim, planes, layout="azim_major")}
                    got_all = T.topo_parameters(azim, planes, tilt, layout="azim_major")
                    pair = T.topo_parameters(azim, planes, tilt, which=("vsf", "openness"), layout="azim_major")
                for name in ALL:
                    assert same_words(got[name], ref[name]), (name, wide, chunk)
                    assert same_words(got_all[name], ref_all[name]), (name, wide, chunk)
                    assert same_words(got_all[name], ref[name]), (name, wide, chunk)
                assert sorted(pair) == ["openness", "vsf"]
                assert same_words(pair["vsf"], ref["vsf"]) and same_words(pair["openness"], ref["openness"])


def test_topo_param_on_device_planes_through_the_c_abi(hip):
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    T = hip.topo_param
    rng = np.random.default_rng(77)
    shape, A = (31, 70), 36
    hori = rng.uniform(-0.3, 1.2, shape + (A,)).astype(np.float32)
    tilt = np.zeros(shape + (3,), np.float32)
    tilt[..., 2] = 1.0
    azim = gridded_azimuths(A)
    ref = T.topo_parameters(azim, hori, tilt)
    d_planes = torch.from_numpy(np.ascontiguousarray(np.transpose(hori, (2, 0, 1)))).to("cuda:0")
    torch.cuda.synchronize()
    out = {n: np.empty(shape, np.float32) for n in ALL}
    with knob(b"planes_chunk", 500, -1):
        _lib.check(_lib.lib().hz_topo_params_planes(azim.ctypes.data, d_planes.data_ptr(), tilt.ctypes.data, shape[0], shape[1], A,
                                                    out["svf"].ctypes.data, out["vsf"].ctypes.data,
                                                    out["openness"].ctypes.data, 0))
    for name in ALL:
        assert same_words(out[name], ref[name]), name
