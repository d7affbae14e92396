"""Terrain.accumulate: weighted sums of sw_dir_cor and of sunlit time over many sun positions, reduced on the device.
The yardstick is the NumPy reduction of shadow_batch / sw_dir_cor_batch outputs -- a float64 accumulator, summed in
ascending position order and rounded to float32 once -- which the kernels must match bit for bit."""
import numpy as np
import pytest

from horayzon_amd import synth
from tests import cases

pytestmark = pytest.mark.gpu


class accum_chunk:
    """hz_debug_set("accum_chunk", k) for the block, the default restored afterwards."""

    def __init__(self, k):
        self.k = k

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"accum_chunk", self.k))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"accum_chunk", -1))
        return False


def _rough(hip, refrac=False, fill=np.nan, scene=False):
    g = cases.rough_terrain(90, 90, seed=31, offset=5, relief=1500.0)
    vec_tilt, vec_norm, enl, elev, mask = cases.terrain_inputs(g)
    mask[20:30, 40:70] = 0
    mask[::11, ::7] = 0
    t = hip.shadow.Terrain()
    extra = {}
    if scene:
        extra["scene"] = hip.Scene.create(g["vert_grid"], 90, 90)
    t.initialise(g["vert_grid"], 90, 90, 5, 5, vec_tilt, vec_norm, enl, elev, mask, refrac_cor=refrac,
                 sw_dir_cor_fill=fill, **extra)
    suns, _, _ = synth.sun_positions(num=48)
    return t, suns, mask, fill


def _hill(hip, refrac=False, fill=-9.0):
    g = cases.c2_hill(height=1500.0)
    vec_tilt, vec_norm, enl, elev, mask = cases.terrain_inputs(g)
    mask[5:9, 5:20] = 0
    mask[100:104, 60:64] = 0
    t = hip.shadow.Terrain()
    t.initialise(g["vert_grid"], 200, 200, 10, 10, vec_tilt, vec_norm, enl, elev, mask, refrac_cor=refrac,
                 sw_dir_cor_fill=fill)
    suns, _, _ = synth.sun_positions(num=24)
    suns = suns + np.array([5000.0, 5000.0, 0.0], np.float32)
    return t, suns, mask, fill


def _weights(kind, n, seed=7):
    if kind == "unit":
        return None
    w = np.random.default_rng(seed).uniform(0.05, 3.0, n).astype(np.float32)
    w[::5] = 0.0
    return w


def reduction(t, suns, weights, mask, fill):
    """float64, ascending s, one rounding: the contract, from the per-position batch maps."""
    n = suns.shape[0]
    sh = np.empty((n,) + mask.shape, np.uint8)
    sw = np.empty((n,) + mask.shape, np.float32)
    t.shadow_batch(suns, sh)
    rays_sh = t.last_stats["num_rays"]
    t.sw_dir_cor_batch(suns, sw)
    rays_sw = t.last_stats["num_rays"]
    w = np.ones(n) if weights is None else weights.astype(np.float64)
    acc_sw = np.zeros(mask.shape)
    acc_lit = np.zeros(mask.shape)
    for s in range(n):
        acc_sw += w[s] * sw[s].astype(np.float64)
        acc_lit += w[s] * (sh[s] == 0)
    ref_sw, ref_lit = acc_sw.astype(np.float32), acc_lit.astype(np.float32)
    ref_sw[mask != 1] = fill
    ref_lit[mask != 1] = fill
    return ref_sw, ref_lit, rays_sh, rays_sw


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) \
        and np.array_equal(np.isnan(a), np.isnan(b))


def accumulate(t, suns, weights, sw=True, lit=True, shape=None):
    out_sw = np.full(shape, 123.0, np.float32) if sw else None
    out_lit = np.full(shape, 123.0, np.float32) if lit else None
    t.accumulate(suns, weights, sw_dir_cor_sum=out_sw, sunlit_sum=out_lit)
    return out_sw, out_lit, dict(t.last_stats)


@pytest.mark.parametrize("case", ("rough", "hill"))
@pytest.mark.parametrize("refrac", (False, True))
@pytest.mark.parametrize("wkind", ("unit", "random"))
def test_matches_the_reduction_of_the_batch_maps(hip, case, refrac, wkind):
    t, suns, mask, fill = (_rough if case == "rough" else _hill)(hip, refrac=refrac)
    w = _weights(wkind, suns.shape[0])
    ref_sw, ref_lit, rays_sh, rays_sw = reduction(t, suns, w, mask, fill)
    assert (ref_lit[mask == 1] > 0).any() and (ref_sw[mask == 1] > 0).any()
    sw, lit, st = accumulate(t, suns, w, shape=mask.shape)
    assert same(sw, ref_sw) and same(lit, ref_lit)
    assert st["num_rays"] == rays_sh
    m = mask != 1
    if np.isnan(fill):
        assert np.isnan(sw[m]).all() and np.isnan(lit[m]).all()
    else:
        assert (sw[m] == np.float32(fill)).all() and (lit[m] == np.float32(fill)).all()
    # one output alone: the same map; the correction alone traces the sw_dir_cor ray set
    sw1, _, st1 = accumulate(t, suns, w, lit=False, shape=mask.shape)
    assert same(sw1, ref_sw) and st1["num_rays"] == rays_sw
    _, lit1, st2 = accumulate(t, suns, w, sw=False, shape=mask.shape)
    assert same(lit1, ref_lit) and st2["num_rays"] == rays_sh
    assert rays_sw < rays_sh


def test_chunk_size_does_not_change_the_maps(hip):
    t, suns, mask, fill = _rough(hip, refrac=True)
    w = _weights("random", suns.shape[0], seed=3)
    base_sw, base_lit, st = accumulate(t, suns, w, shape=mask.shape)
    for k in (1, 3, 7):
        with accum_chunk(k):
            sw, lit, stk = accumulate(t, suns, w, shape=mask.shape)
        assert same(sw, base_sw) and same(lit, base_lit), k
        assert stk["num_rays"] == st["num_rays"]
        with accum_chunk(k):
            sw1, _, _ = accumulate(t, suns, w, lit=False, shape=mask.shape)
        assert same(sw1, base_sw), k


def test_more_positions_than_one_launch_holds(hip):
    """S = 40000 > 32768, the grid.y limit of one batch launch."""
    g = cases.rough_terrain(30, 28, seed=12, offset=4, relief=1200.0)
    vec_tilt, vec_norm, enl, elev, mask = cases.terrain_inputs(g)
    mask[3:5, 3:9] = 0
    t = hip.shadow.Terrain()
    t.initialise(g["vert_grid"], 30, 28, 4, 4, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-1.0)
    suns, _, _ = synth.sun_positions(num=40000)
    w = _weights("random", 40000, seed=11)
    ref_sw, ref_lit, rays_sh, _ = reduction(t, suns, w, mask, -1.0)
    sw, lit, st = accumulate(t, suns, w, shape=mask.shape)
    assert same(sw, ref_sw) and same(lit, ref_lit)
    assert st["num_rays"] == rays_sh


def test_scratch_does_not_grow_with_the_positions(hip):
    t, _, mask, _ = _rough(hip)
    suns, _, _ = synth.sun_positions(num=512)
    _, _, st8 = accumulate(t, suns[::64].copy(), None, shape=mask.shape)
    _, _, st512 = accumulate(t, suns, None, shape=mask.shape)
    assert st8["scratch_bytes"] > 0
    assert st8["scratch_bytes"] == st512["scratch_bytes"]


def test_device_buffers_give_the_same_maps(hip):
    torch = pytest.importorskip("torch")
    t, suns, mask, fill = _rough(hip, refrac=True)
    w = _weights("random", suns.shape[0], seed=5)
    ref_sw, ref_lit, _ = accumulate(t, suns, w, shape=mask.shape)
    dev = "cuda:%d" % t.device
    d_sun, d_w = torch.from_numpy(suns).to(dev), torch.from_numpy(w).to(dev)
    d_sw = torch.full(mask.shape, 7.0, dtype=torch.float32, device=dev)
    d_lit = torch.full(mask.shape, 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t.accumulate(d_sun, d_w, sw_dir_cor_sum=d_sw, sunlit_sum=d_lit)
    torch.cuda.synchronize()
    assert same(d_sw.cpu().numpy(), ref_sw) and same(d_lit.cpu().numpy(), ref_lit)
    # host positions into HBM outputs, and device positions into NumPy outputs
    d_sw.fill_(7.0)
    torch.cuda.synchronize()
    t.accumulate(suns, w, sw_dir_cor_sum=d_sw)
    torch.cuda.synchronize()
    assert same(d_sw.cpu().numpy(), ref_sw)
    out = np.empty(mask.shape, np.float32)
    t.accumulate(d_sun, w, sunlit_sum=out)
    assert same(out, ref_lit)
    # several chunks, each input from its own side: positions in HBM with host weights, and the other way round
    for pos, wts in ((d_sun, w), (suns, d_w)):
        with accum_chunk(2):
            sw, lit = np.full(mask.shape, 7.0, np.float32), np.full(mask.shape, 7.0, np.float32)
            t.accumulate(pos, wts, sw_dir_cor_sum=sw, sunlit_sum=lit)
        assert same(sw, ref_sw) and same(lit, ref_lit)


def test_terrain_on_a_shared_scene(hip):
    t, suns, mask, fill = _rough(hip)
    ts, _, _, _ = _rough(hip, scene=True)
    w = _weights("random", suns.shape[0], seed=9)
    a_sw, a_lit, a_st = accumulate(t, suns, w, shape=mask.shape)
    b_sw, b_lit, b_st = accumulate(ts, suns, w, shape=mask.shape)
    assert same(a_sw, b_sw) and same(a_lit, b_lit)
    assert a_st["num_rays"] == b_st["num_rays"]


def test_band_of_the_c3_tile(hip):
    """256 rows of the 3601^2 tile, the 144 positions of one day."""
    n, off, r0, rows = 3601, 16, 1500, 256
    g = synth.fractal_tile(n=n, offset=off)
    in1 = n - 2 * off
    vec_tilt, enl = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], off)
    vec_tilt = np.ascontiguousarray(vec_tilt[r0:r0 + rows])
    enl = np.ascontiguousarray(enl[r0:r0 + rows])
    vec_norm, _ = synth.planar_frames(rows, in1)
    elev = np.ascontiguousarray(g["z"][off + r0:off + r0 + rows, off:off + in1], np.float32)
    mask = np.ones((rows, in1), np.uint8)
    mask[40:60, 100:900] = 0
    t = hip.shadow.Terrain()
    t.initialise(g["vert_grid"], n, n, off + r0, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-7.0)
    suns, _, _ = synth.sun_positions(num=144)
    w = np.full(144, 600.0, np.float32)                      # 10-minute steps in seconds
    ref_sw, ref_lit, rays_sh, _ = reduction(t, suns, w, mask, -7.0)
    sw, lit, st = accumulate(t, suns, w, shape=mask.shape)
    assert same(sw, ref_sw) and same(lit, ref_lit)
    assert st["num_rays"] == rays_sh
    assert (lit[mask == 1] > 0).mean() > 0.5
