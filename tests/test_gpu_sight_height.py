"""Terrain.sight_height on the GPU: every case bit for bit against the CPU yardstick (tests/sight_height_reference.py: the
NumPy float32 search and the oracle's rays) -- the heights, their minimum over observers and the cells reached as uint32 /
int64 words, so NaN and +inf patterns count, and the number of rays."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from horayzon_amd.shadow import sight_heights
from tests import cases
from tests import sight_height_reference as sr
from tests.test_gpu_viewshed import MAX_POS, fast_cap, six_observers, terrain
from tests.test_viewshed_reference import MAX_DIST, fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS, INF_BITS = 0x7fc00000, 0x7f800000


def reference(g, arrays, obs, heights, **kw):
    vec_tilt, vec_norm, enl, elev, mask = arrays
    ref = sr.sight_height(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_norm, mask, obs,
                          heights, **kw)
    for a in ref[:3]:
        a.setflags(write=False)
    return ref


def run(t, obs, heights, shape, want=(True, True, True), **kw):
    """(height, lowest, cells_reached, stats) into NumPy buffers filled with junk; None for an output not asked for."""
    n = obs.shape[0]
    height = np.full((n,) + shape, -77.0, np.float32) if want[0] else None
    lowest = np.full(shape, -77.0, np.float32) if want[1] else None
    cells = np.full(n, -77, np.int64) if want[2] else None
    t.sight_height(obs, heights, height=height, lowest=lowest, cells_reached=cells, **kw)
    return height, lowest, cells, dict(t.last_stats)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(got, ref):
    height, lowest, cells, st = got
    height_ref, lowest_ref, cells_ref, rays = ref
    print("rays %d / %d, height words differing %s, lowest words differing %s, cells_reached differing %s" % (
        st["num_rays"], rays, None if height is None else int((words(height) != words(height_ref)).sum()),
        None if lowest is None else int((words(lowest) != words(lowest_ref)).sum()),
        None if cells is None else int((cells != cells_ref).sum())))
    if height is not None:
        assert height.dtype == np.float32 and np.array_equal(words(height), words(height_ref))
    if lowest is not None:
        assert lowest.dtype == np.float32 and np.array_equal(words(lowest), words(lowest_ref))
    if cells is not None:
        assert cells.dtype == np.int64 and np.array_equal(cells, cells_ref)
    assert st["num_rays"] == rays


def table_of(n):
    """Tables of the lengths the search treats differently: one entry (no bottom ray), two (no bisection), three (one step),
    130 (not a power of two plus one) and 65535 (the limit of the 16 + 16 bit bracket; 4 mm steps stay distinct in float32
    up to 262 m, where neighbouring floats are 0.03 mm apart)."""
    if n == 1:
        return np.array([0.05], np.float32)
    if n == 2:
        return np.array([0.05, 300.0], np.float32)
    if n == 3:
        return np.array([0.05, 40.0, 300.0], np.float32)
    if n == 130:
        table = sight_heights(258.05, 2.0)
    else:
        assert n == 65535
        table = sight_heights(0.05 + 65534 * 0.004 - 0.002, 0.004)
    assert table.size == n
    return table


@pytest.fixture(scope="module")
def small(hip):
    """The 40 x 40 fixture of the CPU tests, the six observers of the viewshed's GPU tests (the sixth on a DEM vertex), a
    Terrain, and the reference of both tables with and without max_dist."""
    g, *arrays = fixture()
    obs = six_observers(g)
    tables = {n: sight_heights(256.05, acc) for acc, n in ((2.0, 129), (0.25, 1025))}
    refs = {(n, max_dist): reference(g, arrays, obs, tables[n], max_dist=max_dist)
            for n in tables for max_dist in (None, MAX_DIST)}
    return g, arrays, obs, terrain(hip, g, arrays), tables, refs


@pytest.mark.parametrize("max_dist", (None, MAX_DIST))
@pytest.mark.parametrize("n", (129, 1025))
def test_both_tables(small, n, max_dist):
    g, arrays, obs, t, tables, refs = small
    ref = refs[(n, max_dist)]
    on = arrays[4] == 1
    kinds = [int((ref[0][:, on] == tables[n][0]).sum()), int(np.isinf(ref[0][:, on]).sum()),
             int((np.isfinite(ref[0][:, on]) & (ref[0][:, on] > tables[n][0])).sum())]
    print("H[0] %d, +inf %d, between %d" % tuple(kinds))
    assert min(kinds) > (20 if max_dist else 500) and np.isnan(ref[0][:, ~on]).all()
    check(run(t, obs, tables[n], on.shape, max_dist=max_dist), ref)


def test_no_limit_spellings(small):
    g, arrays, obs, t, tables, refs = small
    check(run(t, obs, tables[129], arrays[4].shape, max_dist=float("inf")), refs[(129, None)])


@pytest.mark.parametrize("n", (1, 2, 3, 130, 65535))
def test_table_lengths(small, n):
    g, arrays, obs, t, tables, refs = small
    table = table_of(n)
    for max_dist in (None, MAX_DIST):
        ref = reference(g, arrays, obs, table, max_dist=max_dist)
        if n > 1:
            idx = sr.index_of(ref[0], table)
            assert (idx == 0).any() and (idx == -1).any() and (idx == n - 1).any() and len(np.unique(idx)) >= min(n, 50) + 1
        check(run(t, obs, table, arrays[4].shape, max_dist=max_dist), ref)


def test_one_entry_is_the_viewshed_without_the_facing_test(small):
    """Against the GPU viewshed of the same Terrain: finite <=> code 0, +inf <=> code 2 (4 with max_dist), NaN <=> code 3."""
    g, arrays, obs, t, tables, refs = small
    shape = arrays[4].shape
    table = table_of(1)
    for max_dist in (None, MAX_DIST):
        codes = np.empty((obs.shape[0],) + shape, np.uint8)
        cells_seen = np.empty(obs.shape[0], np.int64)
        t.viewshed(obs, visible=codes, cells_seen=cells_seen, target_elev=0.05, facing=False, max_dist=max_dist)
        rays = t.last_stats["num_rays"]
        height, lowest, cells, st = run(t, obs, table, shape, max_dist=max_dist)
        w = words(height)
        assert np.array_equal(w == words(table)[0], codes == 0)
        assert np.array_equal(w == INF_BITS, (codes == 2) | (codes == 4)) and ((codes == 4).any() == (max_dist is not None))
        assert np.array_equal(w == NAN_BITS, codes == 3)
        assert st["num_rays"] == rays and np.array_equal(cells, cells_seen)
        assert np.array_equal(words(lowest) == words(table)[0], (codes == 0).any(axis=0))


def test_every_subset_of_the_outputs_in_hbm_and_numpy(small):
    """The words do not depend on which outputs are asked for, nor on where they and the observers live."""
    torch = pytest.importorskip("torch")
    g, arrays, obs, t, tables, refs = small
    shape, n = arrays[4].shape, obs.shape[0]
    table, ref = tables[129], refs[(129, MAX_DIST)]
    dev = "cuda:%d" % t.device
    d_obs = torch.from_numpy(obs).to(dev)
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            continue
        check(run(t, obs, table, shape, want, max_dist=MAX_DIST), ref)
        height = torch.full((n,) + shape, -77.0, dtype=torch.float32, device=dev) if want[0] else None
        lowest = torch.full(shape, -77.0, dtype=torch.float32, device=dev) if want[1] else None
        cells = torch.full((n,), -77, dtype=torch.int64, device=dev) if want[2] else None
        torch.cuda.synchronize()
        # observers in HBM with the outputs in HBM; observers on the host for the odd subsets
        t.sight_height(d_obs if want[0] == want[1] else obs, table, height=height, lowest=lowest, cells_reached=cells,
                       max_dist=MAX_DIST)
        torch.cuda.synchronize()
        check(tuple(None if b is None else b.cpu().numpy() for b in (height, lowest, cells)) + (dict(t.last_stats),), ref)
    # observers in HBM, outputs on the host
    height, lowest, cells = np.empty((n,) + shape, np.float32), np.empty(shape, np.float32), np.empty(n, np.int64)
    t.sight_height(d_obs, table, height=height, lowest=lowest, cells_reached=cells, max_dist=MAX_DIST)
    check((height, lowest, cells, dict(t.last_stats)), ref)


def test_ragged_grid_with_tilted_frames(hip):
    """35 x 33 inner cells: partial 16 x 16 tiles in both directions; normals that are not the z axis, so the target points of
    one cell do not lie above each other."""
    g = cases.rough_terrain(43, 41, seed=17, offset=4, relief=1200.0, tilt_frames=True)
    vec_tilt, _, enl, elev, mask = cases.terrain_inputs(g)
    mask[30:, 5:9] = 0
    mask[::9, ::5] = 0
    arrays = (vec_tilt, g["vec_norm"], enl, elev, mask)
    assert mask.shape == (35, 33) and np.abs(g["vec_norm"][..., 0]).max() > 1e-3
    x, y, z = g["x"], g["y"], g["z"]
    obs = np.array([[x[12], y[30], z[30, 12] + 3.0], [x[40], y[42], z[42, 40] + 1.0], [x[20] + 11.0, y[21] - 4.0, z.max() + 40.0],
                    [x[0] - 300.0, y[0] + 200.0, z.mean()], [x[25], y[8], z[8, 25] + 25.0]], np.float32)
    t = terrain(hip, g, arrays)
    table = sight_heights(200.0, 0.5)
    for max_dist in (None, 500.0):
        ref = reference(g, arrays, obs, table, max_dist=max_dist)
        idx = sr.index_of(ref[0], table)
        assert (idx == 0).sum() > 100 and (idx == -1).sum() > 100 and (idx > 0).sum() > 100
        check(run(t, obs, table, mask.shape, max_dist=max_dist), ref)


def test_several_blocks_per_wave(hip):
    """180 x 180 inner cells (144 tiles) and 192 observers: the launch gives every wave two 8 x 8 blocks, so finished lanes take
    cells of the second block while their neighbours are in the middle of a search."""
    g = cases.c2_hill(1500.0)
    arrays = cases.terrain_inputs(g)
    mask = arrays[4]
    mask[50:54, 20:90] = 0
    x, y, z = g["x"], g["y"], g["z"]
    ang = 2.0 * np.pi * np.arange(192) / 192.0
    jj = np.rint(100 + 55 * np.cos(ang)).astype(int)
    ii = np.rint(100 + 55 * np.sin(ang)).astype(int)
    above = np.linspace(2.0, 50.0, 192)
    obs = np.ascontiguousarray(np.stack([x[jj], y[ii], z[ii, jj] + above], axis=1), np.float32)
    # the blocks per wave are the launcher's choice (shadow_config, hz_shadow.hip): its rule, restated here for this shape
    src = open(os.path.join(ROOT, "horayzon_amd", "csrc", "hz_shadow.hip")).read()
    assert "int nb = (int)(wgs / (48.0 * 256.0));" in src and "nb = std::max(1, std::min(std::min(nb, 32), tiles_j));" in src
    tiles_i, tiles_j = (mask.shape[0] + 15) // 16, (mask.shape[1] + 15) // 16
    nb = max(1, min(int(tiles_i * tiles_j * obs.shape[0] / (48.0 * 256.0)), 32, tiles_j))
    nb = next((c for c in range(nb, max(1, nb * 3 // 4) - 1, -1) if tiles_j % c == 0), nb)
    assert (tiles_i, tiles_j) == (12, 12) and nb == 2
    t = terrain(hip, g, arrays)
    table = sight_heights(64.05, 4.0)
    assert table.size == 17
    ref = reference(g, arrays, obs, table, max_dist=4000.0)
    idx = sr.index_of(ref[0], table)
    assert (idx == 0).sum() > 10000 and (idx == -1).sum() > 10000 and (idx > 0).sum() > 10000
    check(run(t, obs, table, mask.shape, max_dist=4000.0), ref)


def test_stack_disciplines_and_counting_give_the_same_words(small):
    g, arrays, obs, t, tables, refs = small
    table, ref = tables[129], refs[(129, None)]
    shape = arrays[4].shape
    try:
        with fast_cap(5):                # below the tree's height on this fixture the launcher takes the level stack, as with 0
            check(run(t, obs, table, shape), ref)
        with fast_cap(0):                # the level-stack instantiation
            check(run(t, obs, table, shape), ref)
        t.count_work(True)
        got = run(t, obs, table, shape)
        check(got, ref)
        assert got[3]["nodes_visited"] > 0 and got[3]["tris_tested"] > 0
        with fast_cap(5):
            check(run(t, obs, table, shape), ref)
        with fast_cap(0):
            check(run(t, obs, table, shape), ref)
    finally:
        t.count_work(False)
    got = run(t, obs, table, shape)
    check(got, ref)
    assert got[3]["nodes_visited"] == 0


def test_overflowed_rays_are_traced_again_inside_a_search(small):
    """The in-kernel retry: with as few fast-stack entries as the launcher accepts for the fast stack (fast_cap >= 5 and >= the
    tree's height, shadow_config) most rays run out of entries and are traced again with the level stack, in the middle of a
    cell's search: the same words.  That the retry ran shows in the node visits: a ray traced twice visits the nodes of both
    traversals."""
    g, arrays, obs, t, tables, refs = small
    shape = arrays[4].shape
    run(t, obs[:1].copy(), tables[129], shape)
    height = t.last_stats["bvh_height"]
    cap = max(5, height)
    assert height >= 1 and cap >= 5 and cap >= height and cap < 19      # the fast stack stays on, with fewer entries than the default's 19
    print("bvh_height %d, cap %d" % (height, cap))
    visits = {}
    try:
        t.count_work(True)
        for n, max_dist in ((129, None), (1025, None), (129, MAX_DIST)):
            ref = refs[(n, max_dist)]
            got = run(t, obs, tables[n], shape, max_dist=max_dist)
            check(got, ref)
            with fast_cap(cap):
                low = run(t, obs, tables[n], shape, max_dist=max_dist)
            check(low, ref)
            with fast_cap(0):
                level = run(t, obs, tables[n], shape, max_dist=max_dist)
            check(level, ref)
            visits[(n, max_dist)] = (got[3]["nodes_visited"], low[3]["nodes_visited"], level[3]["nodes_visited"])
            print("nodes visited: default cap %d, cap %d: %d, level stack %d" % (visits[(n, max_dist)][0], cap,
                                                                               visits[(n, max_dist)][1], visits[(n, max_dist)][2]))
    finally:
        t.count_work(False)
    for default, low, level in visits.values():
        assert low > default
    with fast_cap(cap):                  # the production instantiation at the low cap
        check(run(t, obs, tables[129], shape), refs[(129, None)])
        check(run(t, obs, tables[1025], shape, max_dist=MAX_DIST), refs[(1025, MAX_DIST)])


def test_more_observers_than_one_launch_holds(hip):
    """MAX_POS + 40 observers on an 8 x 8 domain, five distinct ones tiled: a wrong chunk offset in any output shows, and the
    minimum over observers and the cells reached do not depend on where the launches are cut."""
    g = cases.rough_terrain(12, 12, seed=5, offset=2, relief=600.0)
    arrays = cases.terrain_inputs(g)
    mask = arrays[4]
    assert mask.shape == (8, 8)
    mask[2:4, 5:7] = 0
    x, y, z = g["x"], g["y"], g["z"]
    five = np.array([[x[6], y[6], z[6, 6] + 2.0], [x[3], y[9], z[9, 3] + 8.0], [x[10], y[3], z[3, 10] + 1.0],
                     [x[5] + 5.0, y[5] + 5.0, z.max() + 100.0], [x[0] - 100.0, y[11] - 60.0, z.min() + 20.0]], np.float32)
    table = sight_heights(128.05, 1.0)
    height5, lowest5, cells5, rays5 = reference(g, arrays, five, table)
    per_obs = [reference(g, arrays, five[i:i + 1], table)[3] for i in range(5)]
    assert sum(per_obs) == rays5
    assert len({h.tobytes() for h in height5}) == 5
    n = MAX_POS + 40
    idx = np.arange(n) % 5
    obs = np.ascontiguousarray(five[idx])
    times = np.bincount(idx, minlength=5)
    t = terrain(hip, g, arrays)
    height, lowest, cells, st = run(t, obs, table, mask.shape)
    assert np.array_equal(cells, cells5[idx])
    assert np.array_equal(words(lowest), words(lowest5))
    assert np.array_equal(words(height[:5]), words(height5))
    assert np.array_equal(words(height[MAX_POS - 3:MAX_POS + 2]), words(height5[idx[MAX_POS - 3:MAX_POS + 2]]))
    assert np.array_equal(words(height), words(height5[idx]))
    assert st["num_rays"] == int((np.array(per_obs) * times).sum())
    # without the map per observer: the same words from the two small outputs alone
    _, lowest_only, cells_only, st_only = run(t, obs, table, mask.shape, (False, True, True))
    assert np.array_equal(words(lowest_only), words(lowest5)) and np.array_equal(cells_only, cells5[idx])
    assert st_only["num_rays"] == st["num_rays"]


def test_scratch_does_not_grow_with_the_observers(small):
    g, arrays, obs, t, tables, refs = small
    shape = arrays[4].shape
    one = reference(g, arrays, obs[:1], tables[129])
    got1 = run(t, obs[:1].copy(), tables[129], shape)
    check(got1, one)
    many = np.ascontiguousarray(np.tile(obs, (11, 1))[:64])
    got64 = run(t, many, tables[129], shape)
    assert many.shape[0] == 64 and got1[3]["scratch_bytes"] == got64[3]["scratch_bytes"]
    assert np.array_equal(words(got64[1]), words(refs[(129, None)][1]))
    assert np.array_equal(words(got64[0][:6]), words(refs[(129, None)][0])) and np.array_equal(got64[2][6:12], refs[(129, None)][2])


def test_refraction_is_never_applied(hip, small):
    g, arrays, obs, t, tables, refs = small
    tr = terrain(hip, g, arrays, refrac=True)
    check(run(tr, obs, tables[129], arrays[4].shape), refs[(129, None)])
    check(run(tr, obs, tables[1025], arrays[4].shape, max_dist=MAX_DIST), refs[(1025, MAX_DIST)])


def test_c_entry_point_checks_the_table(small):
    """The library's own rules for the table, for callers that do not come through Python: nothing is written."""
    from horayzon_amd import _lib
    g, arrays, obs, t, tables, refs = small
    L = _lib.lib()
    lowest = np.full(arrays[4].shape, -77.0, np.float32)

    def call(table, n=None):
        table = np.ascontiguousarray(table, np.float32)
        return L.hz_terrain_sight_height(t._h, obs.ctypes.data, obs.shape[0], table.ctypes.data, table.size if n is None else n,
                                         0.0, None, lowest.ctypes.data, None, None)
    for table, pattern in (([0.004, 1.0], b"0.005"), ([np.nan, 1.0], b"0.005"), ([0.05, np.inf], b"non-finite"),
                           ([0.05, np.nan, 3.0], b"non-finite"), ([0.05, 1.0, 1.0], b"strictly increasing"),
                           ([0.05, 2.0, 1.0], b"strictly increasing")):
        assert call(table) == 1
        assert pattern in L.hz_last_error()
    for n in (0, -1, 65536):
        assert call([0.05, 1.0], n) == 1 and b"1 to 65535" in L.hz_last_error()
    assert (lowest == -77.0).all()
    assert call([0.05, 1.0]) == 0 and not (lowest == -77.0).any()
