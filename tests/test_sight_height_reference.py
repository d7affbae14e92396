"""The CPU yardstick of Terrain.sight_height (tests/sight_height_reference.py) held to what is already trusted: a linear scan
of the whole table, the oracle's brute-force mode, the viewshed yardstick for a one-entry table and for max_dist, and pinned
counts so that the fixture the GPU tests share cannot go trivial.  The fixture is the viewshed tests': the 40 x 40 rough
terrain, 994 unmasked cells, five observers."""
import numpy as np
import pytest

from horayzon_amd.shadow import sight_heights
from oracle import oracle as orc
from tests import sight_height_reference as sr
from tests import viewshed_reference as vr
from tests.test_viewshed_reference import MAX_DIST, fixture, near_observers

# (height_acc, entries) of the two tables sight_heights(256.05, acc)
TABLES = ((2.0, 129), (0.25, 1025))


def reference(g, vec_norm, mask, observers, heights, **kw):
    return sr.sight_height(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_norm, mask,
                           observers, heights, **kw)


@pytest.fixture(scope="module")
def near():
    g, vec_tilt, vec_norm, enl, elev, mask = fixture()
    obs = near_observers(g)
    scene = orc.Scene(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"])
    refs = {}
    for acc, n in TABLES:
        table = sight_heights(256.05, acc)
        assert table.size == n and table.dtype == np.float32
        refs[n] = (table, reference(g, vec_norm, mask, obs, table, scene=scene))
        for a in refs[n][1][:3]:
            a.setflags(write=False)
    return g, vec_tilt, vec_norm, mask, obs, scene, refs


@pytest.mark.parametrize("n", [n for _, n in TABLES])
def test_bisection_equals_a_linear_scan(near, n):
    """On this fixture visibility is monotone in the height for every pair, so the bisected index is the first visible one: the
    cap on differing pairs is 0."""
    g, vec_tilt, vec_norm, mask, obs, scene, refs = near
    table, (height, lowest, cells, rays) = refs[n]
    vis = sr.linear_scan(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_norm, mask, obs,
                         table, scene=scene)
    assert vis.shape == (5, 994, n)
    # visible(k) never turns off again as k grows
    non_monotone = int((vis[:, :, :-1] & ~vis[:, :, 1:]).any(axis=2).sum())
    first = np.where(vis.any(axis=2), vis.argmax(axis=2), -1)
    got = sr.index_of(height, table).reshape(5, -1)[:, (mask == 1).ravel()]
    differing = int((got != first).sum())
    print("n %d: pairs %d, non-monotone %d, differing %d" % (n, first.size, non_monotone, differing))
    assert first.size == 4970
    assert non_monotone == 0
    assert differing == 0


@pytest.mark.parametrize("n,rays_pinned", [(129, 14352), (1025, 17232)])
def test_counts_are_pinned(near, n, rays_pinned):
    g, vec_tilt, vec_norm, mask, obs, scene, refs = near
    table, (height, lowest, cells, rays) = refs[n]
    on = mask == 1
    assert np.isnan(height[:, ~on]).all() and not np.isnan(height[:, on]).any()
    at_bottom = [int((h[on] == table[0]).sum()) for h in height]
    unreached = [int(np.isinf(h[on]).sum()) for h in height]
    between = [int((np.isfinite(h[on]) & (h[on] > table[0])).sum()) for h in height]
    print("n %d: H[0] %s, +inf %s, between %s, rays %d" % (n, at_bottom, unreached, between, rays))
    assert at_bottom == [622, 82, 967, 13, 18]          # the facing=False cells_seen of the viewshed tests
    assert unreached == [6, 494, 0, 897, 911]
    assert between == [366, 418, 27, 84, 65]
    assert rays == rays_pinned
    # 1 ray for +inf, 2 for H[0], 2 + the bisection steps for the rest
    steps = int(np.ceil(np.log2(n - 1)))
    assert rays <= sum(unreached) + 2 * sum(at_bottom) + (2 + steps) * sum(between)
    assert cells.dtype == np.int64 and cells.tolist() == [a + b for a, b in zip(at_bottom, between)]
    assert height.dtype == np.float32 and (height[np.isfinite(height)] > 0).all()


def test_tree_equals_brute_force(near):
    g, vec_tilt, vec_norm, mask, obs, scene, refs = near
    table, a = refs[129]
    for max_dist, ref in ((None, a), (MAX_DIST, reference(g, vec_norm, mask, obs, table, max_dist=MAX_DIST, scene=scene))):
        b = reference(g, vec_norm, mask, obs, table, max_dist=max_dist, mode=orc.MODE_BRUTE, scene=scene)
        for x, y in zip(ref[:3], b[:3]):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        assert ref[3] == b[3]


def test_one_entry_is_the_viewshed_without_the_facing_test(near):
    g, vec_tilt, vec_norm, mask, obs, scene, refs = near
    table = np.array([0.05], np.float32)
    height, lowest, cells, rays = reference(g, vec_norm, mask, obs, table, scene=scene)
    codes, _, cells_seen, rays_view = vr.viewshed(g["vert_grid"], 40, 40, 4, 4, vec_tilt, vec_norm, mask, obs, target_elev=0.05,
                                                  facing=False, scene=scene)
    assert np.array_equal(np.isfinite(height), codes == vr.VISIBLE)
    assert np.array_equal(height[np.isfinite(height)], np.full(int(np.isfinite(height).sum()), table[0]))
    assert np.array_equal(np.isposinf(height), codes == vr.BLOCKED)
    assert np.array_equal(np.isnan(height), codes == vr.MASKED)
    assert rays == rays_view and np.array_equal(cells, cells_seen)


@pytest.mark.parametrize("n", [n for _, n in TABLES])
def test_max_dist(near, n):
    g, vec_tilt, vec_norm, mask, obs, scene, refs = near
    table, (height, lowest, cells, rays) = refs[n]
    lim, lowest_lim, cells_lim, rays_lim = reference(g, vec_norm, mask, obs, table, max_dist=MAX_DIST, scene=scene)
    # the range is judged at the lowest target point: the viewshed's at target_elev = H[0]
    codes, _, _, _ = vr.viewshed(g["vert_grid"], 40, 40, 4, 4, vec_tilt, vec_norm, mask, obs, target_elev=float(table[0]),
                                 max_dist=MAX_DIST, facing=False, scene=scene)
    far = codes == vr.OUT_OF_RANGE
    assert far.sum(axis=(1, 2)).tolist() == [982, 622, 994, 994, 816]
    assert np.isposinf(lim[far]).all()
    assert np.array_equal(lim[~far].view(np.uint32), height[~far].view(np.uint32))
    assert rays_lim < rays


@pytest.mark.parametrize("n", [n for _, n in TABLES])
def test_lowest_is_the_minimum_over_observers(near, n):
    g, vec_tilt, vec_norm, mask, obs, scene, refs = near
    table, (height, lowest, cells, rays) = refs[n]
    on = mask == 1
    assert np.array_equal(lowest[on], np.fmin.reduce(height)[on])
    assert np.isnan(lowest[~on]).all() and not np.isnan(lowest[on]).any()
    assert lowest.dtype == np.float32 and lowest.shape == mask.shape
    assert np.array_equal(lowest[on], height[:, on].min(axis=0))
    assert np.isinf(lowest[on]).sum() == np.isinf(height[:, on]).all(axis=0).sum()
