"""Terrain.sw_dir_cor_coarse: per sun position, the mean of sw_dir_cor and the sunlit fraction over blocks of P0 x P1 cells,
reduced on the device.  The yardstick is a NumPy reduction of the shadow_batch / sw_dir_cor_batch maps -- a float64
accumulator per coarse cell that takes the block's unmasked cells in row-major order, divided by their number in float64 and
rounded to float32 once -- which the kernels must match bit for bit."""
import numpy as np
import pytest

from horayzon_amd import synth
from tests import cases

pytestmark = pytest.mark.gpu


class debug_set:
    """hz_debug_set(key, value) for the block, the default restored afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, -1))
        return False


def accum_chunk(k):
    return debug_set(b"accum_chunk", k)


def coarse_tile(cells):
    return debug_set(b"coarse_tile", cells)


def _pair(P):
    return (P, P) if isinstance(P, int) else tuple(P)


def _rough_mask(mask):
    mask[16:24, 40:48] = 0       # P = 8: coarse cell (2, 5) has no cell
    mask[::27, ::19] = 0
    mask[20:30, 40:70] = 0       # P = (5, 16): coarse cells (4, 3) and (5, 3) have no cell
    mask[:, 3] = 0               # P = (80, 1): coarse cell (0, 3) has no cell
    mask[77, :] = 0              # P = (1, 80): coarse cell (77, 0) has no cell


def _hill_mask(mask):
    mask[24:36, 60:72] = 0       # P = 12: coarse cell (2, 5) has no cell
    mask[5:9, 5:20] = 0
    mask[100:104, 60:64] = 0
    mask[::50, ::37] = 0
    mask[90:99, 100:120] = 0     # P = (9, 20): coarse cell (10, 5) has no cell


def block_counts(mask, P):
    P0, P1 = _pair(P)
    gy, gx = mask.shape[0] // P0, mask.shape[1] // P1
    return (mask == 1).reshape(gy, P0, gx, P1).sum(axis=(1, 3))


def check_mask(mask, P):
    """Of the coarse cells of P: at least one without a cell, several partly masked, most of them full."""
    P0, P1 = _pair(P)
    n = block_counts(mask, P)
    assert (n == 0).sum() >= 1
    assert ((n > 0) & (n < P0 * P1)).sum() >= 5
    assert (n == P0 * P1).sum() > n.size // 2


_scenes = {}


def scene(hip, case, refrac):
    """Terrain, positions, mask, fill and the batch maps of (case, refrac): computed once, never written again."""
    key = (case, refrac)
    if key in _scenes:
        return _scenes[key]
    if case == "rough":
        g = cases.rough_terrain(90, 90, seed=31, offset=5, relief=1500.0)
        n, off, fill, base = 90, 5, np.nan, 8
        suns, _, _ = synth.sun_positions(num=48)
    else:
        g = cases.c2_hill(height=1500.0)
        n, off, fill, base = 200, 10, -9.0, 12
        suns, _, _ = synth.sun_positions(num=24)
        suns = suns + np.array([5000.0, 5000.0, 0.0], np.float32)
    vec_tilt, vec_norm, enl, elev, mask = cases.terrain_inputs(g)
    (_rough_mask if case == "rough" else _hill_mask)(mask)
    check_mask(mask, base)                                   # from the mask alone, before any GPU call
    t = hip.shadow.Terrain()
    t.initialise(g["vert_grid"], n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, refrac_cor=refrac,
                 sw_dir_cor_fill=fill)
    S = suns.shape[0]
    sh = np.empty((S,) + mask.shape, np.uint8)
    sw = np.empty((S,) + mask.shape, np.float32)
    t.shadow_batch(suns, sh)
    rays_sh = t.last_stats["num_rays"]
    t.sw_dir_cor_batch(suns, sw)
    rays_sw = t.last_stats["num_rays"]
    for a in (suns, mask, sh, sw):
        a.setflags(write=False)
    inputs = (g, off, vec_tilt, vec_norm, enl, elev)
    _scenes[key] = dict(t=t, suns=suns, mask=mask, fill=fill, sh=sh, sw=sw, rays_sh=rays_sh, rays_sw=rays_sw, inputs=inputs)
    return _scenes[key]


def block_means(sw, sh, mask, P, fill):
    """The contract from per-position maps sw f32[S][y][x] and sh u8[S][y][x]: (f_cor, sunlit_frac) f32[S][gy][gx]."""
    P0, P1 = _pair(P)
    S = sw.shape[0]
    n = block_counts(mask, P)
    acc = np.zeros((S,) + n.shape, np.float64)
    for di in range(P0):
        for dj in range(P1):
            on = np.broadcast_to(mask[di::P0, dj::P1] == 1, acc.shape)
            np.add(acc, sw[:, di::P0, dj::P1].astype(np.float64), out=acc, where=on)     # masked cells: no add at all
    lit = ((sh == 0) & (mask == 1)).reshape(S, n.shape[0], P0, n.shape[1], P1).sum(axis=(2, 4))
    some = np.broadcast_to(n > 0, acc.shape)
    nn = np.maximum(n, 1).astype(np.float64)
    f_cor = (acc / nn).astype(np.float32)
    frac = (lit.astype(np.float64) / nn).astype(np.float32)
    f_cor[~some] = fill
    frac[~some] = fill
    return f_cor, frac


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) \
        and np.array_equal(np.isnan(a), np.isnan(b))


def coarse(t, suns, P, sw=True, lit=True, prefill=123.0):
    P0, P1 = _pair(P)
    shape = (suns.shape[0], t._shape[0] // P0, t._shape[1] // P1)
    f_cor = np.full(shape, prefill, np.float32) if sw else None
    frac = np.full(shape, prefill, np.float32) if lit else None
    t.sw_dir_cor_coarse(suns, P, f_cor=f_cor, sunlit_frac=frac)
    return f_cor, frac, dict(t.last_stats)


def is_fill(a, fill):
    return np.isnan(a).all() if np.isnan(fill) else (a == np.float32(fill)).all()


PIXELS = {"rough": (8, (5, 16), (80, 1), (1, 80), (80, 80), 1), "hill": (12, (9, 20), (180, 180))}


@pytest.mark.parametrize("refrac", (False, True))
@pytest.mark.parametrize("case", ("rough", "hill"))
def test_matches_the_block_means_of_the_batch_maps(hip, case, refrac):
    sc = scene(hip, case, refrac)
    t, suns, mask, fill = sc["t"], sc["suns"], sc["mask"], sc["fill"]
    for P in PIXELS[case]:
        ref_f, ref_l = block_means(sc["sw"], sc["sh"], mask, P, fill)
        n = np.broadcast_to(block_counts(mask, P), ref_f.shape)
        f_cor, frac, st = coarse(t, suns, P)
        assert same(f_cor, ref_f) and same(frac, ref_l), P
        assert st["num_rays"] == sc["rays_sh"], P
        assert (f_cor[n > 0] > 0).any(), P
        if P != 1:
            assert ((frac[n > 0] > 0) & (frac[n > 0] < 1)).any(), P
        if (n == 0).any():
            assert is_fill(f_cor[n == 0], fill) and is_fill(frac[n == 0], fill), P
        # one output alone: the same table; the correction alone traces the sw_dir_cor ray set
        f1, _, st1 = coarse(t, suns, P, lit=False)
        assert same(f1, ref_f) and st1["num_rays"] == sc["rays_sw"], P
        _, l1, st2 = coarse(t, suns, P, sw=False)
        assert same(l1, ref_l) and st2["num_rays"] == sc["rays_sh"], P
        assert st1["num_rays"] < st2["num_rays"], P
    assert any((block_counts(mask, P) == 0).any() for P in PIXELS[case])


@pytest.mark.parametrize("tile", (64, 7))
def test_tile_of_the_reduction_changes_nothing(hip, tile):
    """Small LDS tiles: several strips per coarse row, one tile row at a time, and blocks wider than the tile (the kernel
    without LDS), on the shapes of the first test."""
    for case in ("rough", "hill"):
        sc = scene(hip, case, True)
        for P in PIXELS[case]:
            ref_f, ref_l = block_means(sc["sw"], sc["sh"], sc["mask"], P, sc["fill"])
            with coarse_tile(tile):
                f_cor, frac, _ = coarse(sc["t"], sc["suns"], P)
                f1, _, _ = coarse(sc["t"], sc["suns"], P, lit=False)
                _, l1, _ = coarse(sc["t"], sc["suns"], P, sw=False)
            assert same(f_cor, ref_f) and same(frac, ref_l), (case, P)
            assert same(f1, ref_f) and same(l1, ref_l), (case, P)


def test_one_cell_per_coarse_cell_is_the_batch_map(hip):
    sc = scene(hip, "rough", True)
    mask, fill = sc["mask"], sc["fill"]
    f_cor, frac, _ = coarse(sc["t"], sc["suns"], 1)
    on = np.broadcast_to(mask == 1, f_cor.shape)
    assert f_cor.shape == sc["sw"].shape
    assert np.array_equal(f_cor[on].view(np.uint32), sc["sw"][on].view(np.uint32))
    assert set(np.unique(frac[on])) == {0.0, 1.0}
    assert np.array_equal(frac[on] == 1.0, sc["sh"][on] == 0)
    assert is_fill(f_cor[~on], fill) and is_fill(frac[~on], fill)


def test_chunk_size_does_not_change_the_tables(hip):
    sc = scene(hip, "rough", True)
    t, suns = sc["t"], sc["suns"]
    base_f, base_l, st = coarse(t, suns, 8)
    base_f1, _, st1 = coarse(t, suns, 8, lit=False)
    for k in (1, 5, 7, 48):
        with accum_chunk(k):
            f_cor, frac, stk = coarse(t, suns, 8)
            f1, _, stk1 = coarse(t, suns, 8, lit=False)
        assert same(f_cor, base_f) and same(frac, base_l) and same(f1, base_f1), k
        assert stk["num_rays"] == st["num_rays"] and stk1["num_rays"] == st1["num_rays"], k
    with accum_chunk(7):
        _, _, st14 = coarse(t, suns[:14].copy(), 8)
        _, _, st48 = coarse(t, suns, 8)
    assert st14["scratch_bytes"] > 0
    assert st14["scratch_bytes"] == st48["scratch_bytes"]


def test_device_buffers_give_the_same_tables(hip):
    torch = pytest.importorskip("torch")
    sc = scene(hip, "rough", True)
    t, suns = sc["t"], sc["suns"]
    ref_f, ref_l, _ = coarse(t, suns, (5, 16))
    dev = "cuda:%d" % t.device
    d_sun = torch.from_numpy(suns.copy()).to(dev)
    d_f = torch.full(ref_f.shape, 7.0, dtype=torch.float32, device=dev)
    d_l = torch.full(ref_f.shape, 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t.sw_dir_cor_coarse(d_sun, (5, 16), f_cor=d_f, sunlit_frac=d_l)
    torch.cuda.synchronize()
    assert same(d_f.cpu().numpy(), ref_f) and same(d_l.cpu().numpy(), ref_l)
    # host positions into HBM outputs, and device positions into NumPy outputs
    d_f.fill_(7.0)
    torch.cuda.synchronize()
    t.sw_dir_cor_coarse(suns, (5, 16), f_cor=d_f)
    torch.cuda.synchronize()
    assert same(d_f.cpu().numpy(), ref_f)
    out = np.empty(ref_l.shape, np.float32)
    t.sw_dir_cor_coarse(d_sun, (5, 16), sunlit_frac=out)
    assert same(out, ref_l)
    with pytest.raises(ValueError, match="device"):
        t.sw_dir_cor_coarse(suns, (5, 16), f_cor=torch.zeros(ref_f.shape, dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        t.sw_dir_cor_coarse(torch.from_numpy(suns.copy()), (5, 16), f_cor=d_f)


def test_against_the_cpu_oracle(hip, orc):
    """Independent of the batch kernels: the yardstick fed from oracle.Terrain.sw_dir_cor / .shadow, one position at a time."""
    sc = scene(hip, "rough", False)
    g, off, vec_tilt, vec_norm, enl, elev = sc["inputs"]
    mask, fill = sc["mask"], sc["fill"]
    suns = np.ascontiguousarray(sc["suns"][4:40:6])
    assert suns.shape[0] == 6
    tc = orc.Terrain()
    tc.initialise(g["vert_grid"], 90, 90, off, off, vec_tilt, vec_norm, enl, elev, np.array(mask), sw_dir_cor_fill=fill)
    sh = np.empty((6,) + mask.shape, np.uint8)
    sw = np.empty((6,) + mask.shape, np.float32)
    for s in range(6):
        tc.shadow(suns[s], sh[s])
        tc.sw_dir_cor(suns[s], sw[s])
    ref_f, ref_l = block_means(sw, sh, mask, 8, fill)
    assert (ref_f[np.isfinite(ref_f)] > 0).any() and ((ref_l > 0) & (ref_l < 1)).any()
    f_cor, frac, _ = coarse(sc["t"], suns, 8)
    assert same(f_cor, ref_f) and same(frac, ref_l)


def test_outputs_are_not_read(hip):
    sc = scene(hip, "hill", False)
    a_f, a_l, _ = coarse(sc["t"], sc["suns"], 12, prefill=123.0)
    b_f, b_l, _ = coarse(sc["t"], sc["suns"], 12, prefill=np.nan)
    assert same(a_f, b_f) and same(a_l, b_l)
    assert not np.isnan(a_f).any() and (a_f != 123.0).all() and (a_l != 123.0).all()       # fill -9.0: every value is written


def test_calls_leave_no_state(hip):
    sc = scene(hip, "hill", True)
    t, suns, mask, fill = sc["t"], sc["suns"], sc["mask"], sc["fill"]
    f_cor, frac, _ = coarse(t, suns, 12)
    ref_f, ref_l = block_means(sc["sw"], sc["sh"], mask, 12, fill)
    assert same(f_cor, ref_f) and same(frac, ref_l)
    acc_sw = np.full(mask.shape, 123.0, np.float32)
    acc_lit = np.full(mask.shape, 123.0, np.float32)
    t.accumulate(suns, sw_dir_cor_sum=acc_sw, sunlit_sum=acc_lit)
    tot_sw, tot_lit = np.zeros(mask.shape), np.zeros(mask.shape)
    for s in range(suns.shape[0]):
        tot_sw += sc["sw"][s].astype(np.float64)
        tot_lit += sc["sh"][s] == 0
    tot_sw, tot_lit = tot_sw.astype(np.float32), tot_lit.astype(np.float32)
    tot_sw[mask != 1] = fill
    tot_lit[mask != 1] = fill
    assert same(acc_sw, tot_sw) and same(acc_lit, tot_lit)
    f_cor, frac, _ = coarse(t, suns, (9, 20))
    ref_f, ref_l = block_means(sc["sw"], sc["sh"], mask, (9, 20), fill)
    assert same(f_cor, ref_f) and same(frac, ref_l)
