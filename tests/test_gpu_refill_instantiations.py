"""Every instantiation of every refill kernel (k_shadow_refill, k_accum_refill, k_viewshed_refill, k_sight_refill; the loop:
hz_refill_loop.inc) through the one launch table (hz_shadow.h: refill_launch, kernels[count][fast]).  Each call runs with
Terrain.count_work off and on and with the fast stack (the default) and the level stack (hz_debug_set("shadow_fast_cap", 0)):
every output word equals the CPU yardstick of the call's own test in all four, the traversal counters are non-zero exactly
when counting is on, and the number of rays does not depend on the instantiation."""
import numpy as np
import pytest

from tests import cases
from tests import sight_height_reference as sr
from tests import viewshed_reference as vr
from tests.debug_knobs import fast_cap

pytestmark = pytest.mark.gpu

FILL = -9.0
COMBINATIONS = tuple((count, cap) for count in (False, True) for cap in (None, 0))      # cap None: the default, the fast stack


def words(a):
    """Floats as their uint32 words (NaN and +inf patterns count), other arrays as they are."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def scene(hip, orc):
    """21 x 37 inner cells (partial 16 x 16 tiles in both directions, several workgroups), a few masked, 1500 m of relief on
    30 m cells; two low suns, two observers, three heights; the Terrain and the references of every call."""
    g = cases.rough_terrain(29, 45, seed=23, offset=4, relief=1500.0)
    vec_tilt, vec_norm, enl, elev, mask = cases.terrain_inputs(g)
    mask[2:4, 5:11] = 0
    mask[17, 30:] = 0
    assert mask.shape == (21, 37)
    args = (g["vert_grid"], 29, 45, 4, 4, vec_tilt, vec_norm, enl, elev, mask)
    tg, tc = hip.shadow.Terrain(), orc.Terrain()
    tg.initialise(*args, sw_dir_cor_fill=FILL)
    tc.initialise(*args, sw_dir_cor_fill=FILL)
    x, y, z = g["x"], g["y"], g["z"]
    mid = np.array([x.mean(), y.mean(), 0.0])
    alt, az = np.deg2rad([12.0, 25.0]), np.deg2rad([100.0, 250.0])
    suns = (mid + 1.0e9 * np.stack([np.cos(alt) * np.sin(az), np.cos(alt) * np.cos(az), np.sin(alt)], axis=1)).astype(np.float32)
    hi = np.unravel_index(np.argmax(z), z.shape)
    obs = np.array([[x[hi[1]], y[hi[0]], z[hi] + 2.0], [x[0] - 300.0, y[0] + 200.0, z.mean()]], np.float32)
    heights = np.array([0.05, 40.0, 300.0], np.float32)
    weights = np.array([0.75, 2.5], np.float32)

    sh, sw = np.empty((2,) + mask.shape, np.uint8), np.empty((2,) + mask.shape, np.float32)
    rays_sh = rays_sw = 0
    for s in range(2):
        tc.shadow(suns[s], sh[s]); rays_sh += tc.rays
        tc.sw_dir_cor(suns[s], sw[s]); rays_sw += tc.rays
    assert all((sh[s] == c).any() for s in range(2) for c in (0, 1, 2, 3)) and rays_sw <= rays_sh
    # Terrain.accumulate's contract (tests/test_gpu_accumulate.py: reduction): float64, ascending position, one rounding
    acc_sw, acc_lit = np.zeros(mask.shape), np.zeros(mask.shape)
    for s in range(2):
        acc_sw += np.float64(weights[s]) * sw[s].astype(np.float64)
        acc_lit += np.float64(weights[s]) * (sh[s] == 0)
    sum_sw, sum_lit = acc_sw.astype(np.float32), acc_lit.astype(np.float32)
    sum_sw[mask != 1] = FILL
    sum_lit[mask != 1] = FILL
    grid = (g["vert_grid"], 29, 45, 4, 4)
    view = vr.viewshed(*grid, vec_tilt, vec_norm, mask, obs)
    assert all((view[0][s] == c).any() for s in range(2) for c in (0, 2, 3))
    sight = sr.sight_height(*grid, vec_norm, mask, obs, heights, max_dist=700.0)
    on = mask == 1
    assert (sight[0][:, on] == heights[0]).any() and np.isinf(sight[0][:, on]).any() and (sight[0][:, on] == heights[1]).any()

    def call(name):
        """The outputs of one call, into buffers filled with junk."""
        u8 = np.full((2,) + mask.shape, 77, np.uint8)
        f32 = np.full((2,) + mask.shape, -77.0, np.float32)
        a, b = np.full(mask.shape, -77.0, np.float32), np.full(mask.shape, -77.0, np.float32)
        if name == "shadow":
            tg.shadow_batch(suns, u8)
            rays = tg.last_stats["num_rays"]
            a8 = np.full(mask.shape, 77, np.uint8)
            tg.shadow(suns[1], a8)
            assert rays > tg.last_stats["num_rays"] > 0
            return (u8, a8), rays
        if name == "sw_dir_cor":
            tg.sw_dir_cor_batch(suns, f32)
            rays = tg.last_stats["num_rays"]
            tg.sw_dir_cor(suns[1], a)
            assert rays > tg.last_stats["num_rays"] > 0
            return (f32, a), rays
        if name == "accumulate_both":
            tg.accumulate(suns, weights, sw_dir_cor_sum=a, sunlit_sum=b)
            return (a, b), tg.last_stats["num_rays"]
        if name == "accumulate_sw_dir_cor":
            tg.accumulate(suns, weights, sw_dir_cor_sum=a)
            return (a,), tg.last_stats["num_rays"]
        cells = np.full(2, -77, np.int64)
        if name == "viewshed":
            seen = np.full(mask.shape, -77, np.int32)
            tg.viewshed(obs, visible=u8, seen_count=seen, cells_seen=cells)
            return (u8, seen, cells), tg.last_stats["num_rays"]
        assert name == "sight_height"
        tg.sight_height(obs, heights, height=f32, lowest=a, cells_reached=cells, max_dist=700.0)
        return (f32, a, cells), tg.last_stats["num_rays"]

    refs = {"shadow": ((sh, sh[1]), rays_sh), "sw_dir_cor": ((sw, sw[1]), rays_sw),
            "accumulate_both": ((sum_sw, sum_lit), rays_sh), "accumulate_sw_dir_cor": ((sum_sw,), rays_sw),
            "viewshed": (view[:3], view[3]), "sight_height": (sight[:3], sight[3])}
    for outs, _ in refs.values():
        for a in outs:
            a.setflags(write=False)
    return tg, call, refs


@pytest.mark.parametrize("name", ("shadow", "sw_dir_cor", "accumulate_both", "accumulate_sw_dir_cor", "viewshed", "sight_height"))
def test_all_four_instantiations(scene, name):
    t, call, refs = scene
    want, rays = refs[name]
    try:
        for count, cap in COMBINATIONS:
            t.count_work(count)
            if cap is None:
                got, n = call(name)
            else:
                with fast_cap(cap):
                    got, n = call(name)
            st = dict(t.last_stats)
            print("%s count %d cap %s: rays %d / %d, nodes %d, tris %d, words differing %s" % (
                name, count, cap, n, rays, st["nodes_visited"], st["tris_tested"],
                [int((words(a) != words(b)).sum()) for a, b in zip(got, want)]))
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(words(a), words(b))
            assert n == rays
            assert (st["nodes_visited"] > 0) == count and (st["tris_tested"] > 0) == count
            # the default cap is the fast stack: min(19, 3 * height + 1) >= max(5, height) (shadow_config, hz_shadow.hip)
            assert 2 <= st["bvh_height"] <= 19
    finally:
        t.count_work(False)
