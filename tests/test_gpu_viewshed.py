"""Terrain.viewshed on the GPU: every case bit for bit against the CPU yardstick (tests/viewshed_reference.py: the NumPy
float32 classification and the oracle's rays) -- the codes, both counts and the number of rays."""
import itertools
import os

import numpy as np
import pytest

from horayzon_amd import synth
from tests import cases
from tests import viewshed_reference as vr
from tests.debug_knobs import fast_cap
from tests.test_viewshed_reference import MAX_DIST, fixture, near_observers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POS = 32768          # observers of one launch (hz_api_sun.hip: HZ_SHADOW_MAX_POS, grid.y)


def six_observers(g):
    """The five observers of the CPU tests and a sixth exactly on a DEM vertex: rays that end on the surface."""
    on_vertex = vr.vertices(g["vert_grid"], 40, 40)[17 + 4, 9 + 4]
    return np.ascontiguousarray(np.vstack([near_observers(g), on_vertex[None, :]]), np.float32)


def terrain(hip, g, arrays, refrac=False):
    vec_tilt, vec_norm, enl, elev, mask = arrays
    t = hip.shadow.Terrain()
    t.initialise(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_tilt, vec_norm, enl, elev,
                 mask, refrac_cor=refrac)
    return t


def reference(g, arrays, obs, **kw):
    vec_tilt, vec_norm, enl, elev, mask = arrays
    return vr.viewshed(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_tilt, vec_norm, mask,
                       obs, **kw)


def run(t, obs, shape, want=(True, True, True), **kw):
    """(codes, seen_count, cells_seen, stats) into NumPy buffers filled with junk; None for an output not asked for."""
    n = obs.shape[0]
    vis = np.full((n,) + shape, 77, np.uint8) if want[0] else None
    seen = np.full(shape, -77, np.int32) if want[1] else None
    cells = np.full(n, -77, np.int64) if want[2] else None
    t.viewshed(obs, visible=vis, seen_count=seen, cells_seen=cells, **kw)
    return vis, seen, cells, dict(t.last_stats)


def check(got, ref):
    vis, seen, cells, st = got
    codes, seen_ref, cells_ref, rays = ref
    print("rays %d / %d, codes differing %s, seen differing %s, cells_seen differing %s" % (
        st["num_rays"], rays, None if vis is None else int((vis != codes).sum()),
        None if seen is None else int((seen != seen_ref).sum()), None if cells is None else int((cells != cells_ref).sum())))
    if vis is not None:
        assert vis.dtype == np.uint8 and np.array_equal(vis, codes)
    if seen is not None:
        assert seen.dtype == np.int32 and np.array_equal(seen, seen_ref)
    if cells is not None:
        assert cells.dtype == np.int64 and np.array_equal(cells, cells_ref)
    assert st["num_rays"] == rays


@pytest.fixture(scope="module")
def small(hip):
    """The 40 x 40 fixture of the CPU tests, its six observers, a Terrain, and the reference of every flag combination."""
    g, *arrays = fixture()
    obs = six_observers(g)
    refs = {(facing, max_dist): reference(g, arrays, obs, facing=facing, max_dist=max_dist)
            for facing in (True, False) for max_dist in (None, MAX_DIST)}
    for r in refs.values():
        r[0].setflags(write=False); r[1].setflags(write=False); r[2].setflags(write=False)
    return g, arrays, obs, terrain(hip, g, arrays), refs


@pytest.mark.parametrize("max_dist", (None, MAX_DIST))
@pytest.mark.parametrize("facing", (True, False))
def test_near_observers(small, facing, max_dist):
    g, arrays, obs, t, refs = small
    ref = refs[(facing, max_dist)]
    hist = vr.histogram(ref[0])
    assert hist[0] > 50 and hist[2] > 500 and (hist[1] > 500) == facing and (hist[4] > 3000) == (max_dist is not None)
    check(run(t, obs, arrays[4].shape, facing=facing, max_dist=max_dist), ref)


def test_defaults_are_facing_and_no_limit(small):
    g, arrays, obs, t, refs = small
    check(run(t, obs, arrays[4].shape), refs[(True, None)])
    check(run(t, obs, arrays[4].shape, max_dist=float("inf")), refs[(True, None)])


def test_target_elev(small):
    g, arrays, obs, t, refs = small
    ref = reference(g, arrays, obs, target_elev=1.5)
    assert not np.array_equal(ref[0], refs[(True, None)][0])
    check(run(t, obs, arrays[4].shape, target_elev=1.5), ref)


def test_every_subset_of_the_outputs_in_hbm_and_numpy(small):
    """Codes and counts do not depend on which outputs are asked for, nor on where they and the observers live."""
    torch = pytest.importorskip("torch")
    g, arrays, obs, t, refs = small
    shape, n = arrays[4].shape, obs.shape[0]
    ref = refs[(True, MAX_DIST)]
    dev = "cuda:%d" % t.device
    d_obs = torch.from_numpy(obs).to(dev)
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            continue
        check(run(t, obs, shape, want, max_dist=MAX_DIST), ref)
        vis = torch.full((n,) + shape, 77, dtype=torch.uint8, device=dev) if want[0] else None
        seen = torch.full(shape, -77, dtype=torch.int32, device=dev) if want[1] else None
        cells = torch.full((n,), -77, dtype=torch.int64, device=dev) if want[2] else None
        torch.cuda.synchronize()
        # observers in HBM with the outputs in HBM; observers on the host for the odd subsets
        t.viewshed(d_obs if want[0] == want[1] else obs, visible=vis, seen_count=seen, cells_seen=cells, max_dist=MAX_DIST)
        torch.cuda.synchronize()
        check(tuple(None if b is None else b.cpu().numpy() for b in (vis, seen, cells)) + (dict(t.last_stats),), ref)
    # observers in HBM, outputs on the host
    vis, seen, cells = np.empty((n,) + shape, np.uint8), np.empty(shape, np.int32), np.empty(n, np.int64)
    t.viewshed(d_obs, visible=vis, seen_count=seen, cells_seen=cells, max_dist=MAX_DIST)
    check((vis, seen, cells, dict(t.last_stats)), ref)


def test_ragged_grid_with_tilted_frames(hip):
    """35 x 33 inner cells: partial 16 x 16 tiles in both directions; normals that are not the z axis."""
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
    for facing, max_dist in ((True, None), (False, 500.0)):
        ref = reference(g, arrays, obs, facing=facing, max_dist=max_dist)
        hist = vr.histogram(ref[0])
        assert hist[0] > 100 and hist[2] > 100
        check(run(t, obs, mask.shape, facing=facing, max_dist=max_dist), ref)


def test_far_observers_give_the_shadow_batch(small):
    """The existing kernel as a second yardstick: at a sun's distance the codes are shadow's, ray for ray."""
    g, arrays, obs, t, refs = small
    suns, _, _ = synth.sun_positions(num=24)
    shape = arrays[4].shape
    want = np.empty((24,) + shape, np.uint8)
    t.shadow_batch(suns, want)
    rays = t.last_stats["num_rays"]
    vis, seen, cells, st = run(t, suns, shape)
    assert vr.histogram(want)[:4] == [6435, 10051, 7370, 720]
    assert np.array_equal(vis, want) and st["num_rays"] == rays
    assert np.array_equal(cells, (want == 0).sum(axis=(1, 2)))
    assert np.array_equal(seen, np.where(arrays[4] == 1, (want == 0).sum(axis=0), -1))


def test_refraction_is_never_applied(hip, small):
    g, arrays, obs, t, refs = small
    tr = terrain(hip, g, arrays, refrac=True)
    check(run(tr, obs, arrays[4].shape), refs[(True, None)])
    # ... where shadow() does bend the ray: low suns give other codes with refraction
    suns, _, _ = synth.sun_positions(num=24)
    a, b = np.empty((24,) + arrays[4].shape, np.uint8), np.empty((24,) + arrays[4].shape, np.uint8)
    t.shadow_batch(suns, a)
    tr.shadow_batch(suns, b)
    assert not np.array_equal(a, b)
    va, _, _, _ = run(t, suns, arrays[4].shape, (True, False, False))
    vb, _, _, _ = run(tr, suns, arrays[4].shape, (True, False, False))
    assert np.array_equal(va, vb) and np.array_equal(va, a)


def test_stack_disciplines_and_counting_give_the_same_words(small):
    g, arrays, obs, t, refs = small
    ref = refs[(False, None)]
    shape = arrays[4].shape
    try:
        with fast_cap(5):                # below the tree's height on this fixture the launcher takes the level stack, as with 0
            check(run(t, obs, shape, facing=False), ref)
        with fast_cap(0):                # the level-stack instantiation
            check(run(t, obs, shape, facing=False), ref)
        t.count_work(True)
        got = run(t, obs, shape, facing=False)
        check(got, ref)
        assert got[3]["nodes_visited"] > 0 and got[3]["tris_tested"] > 0
        with fast_cap(5):
            check(run(t, obs, shape, facing=False), ref)
        with fast_cap(0):
            check(run(t, obs, shape, facing=False), ref)
    finally:
        t.count_work(False)
    got = run(t, obs, shape, facing=False)
    check(got, ref)
    assert got[3]["nodes_visited"] == 0


def test_overflowed_rays_are_traced_again_with_their_own_tfar(small):
    """The in-kernel retry: with as few fast-stack entries as the launcher accepts for the fast stack (fast_cap >= 5 and
    >= the tree's height, shadow_config) most rays run out of entries and are traced again with the level stack -- with the
    ray's own finite tfar, or the codes of the cells behind an observer change.  That the retry ran shows in the node visits:
    a ray traced twice visits the nodes of both traversals."""
    g, arrays, obs, t, refs = small
    shape = arrays[4].shape
    run(t, obs[:1].copy(), shape)
    height = t.last_stats["bvh_height"]
    cap = max(5, height)
    assert height >= 1 and cap >= 5 and cap >= height and cap < 19      # the fast stack stays on, with fewer entries than the default's 19
    print("bvh_height %d, cap %d" % (height, cap))
    visits = {}
    try:
        t.count_work(True)
        for facing, max_dist in ((False, None), (True, None), (False, MAX_DIST)):
            ref = refs[(facing, max_dist)]
            got = run(t, obs, shape, facing=facing, max_dist=max_dist)
            check(got, ref)
            with fast_cap(cap):
                low = run(t, obs, shape, facing=facing, max_dist=max_dist)
            check(low, ref)
            with fast_cap(0):
                level = run(t, obs, shape, facing=facing, max_dist=max_dist)
            check(level, ref)
            visits[(facing, max_dist)] = (got[3]["nodes_visited"], low[3]["nodes_visited"], level[3]["nodes_visited"])
            print("nodes visited: default cap %d, cap %d: %d, level stack %d" % (visits[(facing, max_dist)][0], cap,
                                                                               visits[(facing, max_dist)][1], visits[(facing, max_dist)][2]))
    finally:
        t.count_work(False)
    # a ray traced twice adds the node visits of its first, abandoned traversal to those of a complete one (for a ray that hits
    # nothing both disciplines visit the same nodes: every node whose box the ray meets)
    for default, low, level in visits.values():
        assert low > default
    with fast_cap(cap):                  # the production instantiation at the low cap
        check(run(t, obs, shape, facing=False), refs[(False, None)])
        check(run(t, obs, shape), refs[(True, None)])


def test_several_blocks_per_wave(hip):
    """180 x 180 inner cells (144 tiles) and 192 observers: the launch gives every wave two 8 x 8 blocks."""
    g = cases.c2_hill(1500.0)
    arrays = cases.terrain_inputs(g)
    mask = arrays[4]
    mask[50:54, 20:90] = 0
    x, y, z = g["x"], g["y"], g["z"]
    ang = 2.0 * np.pi * np.arange(192) / 192.0
    jj = np.rint(100 + 55 * np.cos(ang)).astype(int)
    ii = np.rint(100 + 55 * np.sin(ang)).astype(int)
    height = np.linspace(2.0, 50.0, 192)
    obs = np.ascontiguousarray(np.stack([x[jj], y[ii], z[ii, jj] + height], axis=1), np.float32)
    # the blocks per wave are the launcher's choice (shadow_config, hz_shadow.hip): its rule, restated here for this shape.  If the
    # rule's text moves, this fails and the case is sized again -- it must not turn into one block per wave unnoticed
    src = open(os.path.join(ROOT, "horayzon_amd", "csrc", "hz_shadow.hip")).read()
    assert "int nb = (int)(wgs / (48.0 * 256.0));" in src and "nb = std::max(1, std::min(std::min(nb, 32), tiles_j));" in src
    tiles_i, tiles_j = (mask.shape[0] + 15) // 16, (mask.shape[1] + 15) // 16
    nb = max(1, min(int(tiles_i * tiles_j * obs.shape[0] / (48.0 * 256.0)), 32, tiles_j))
    nb = next((c for c in range(nb, max(1, nb * 3 // 4) - 1, -1) if tiles_j % c == 0), nb)
    assert (tiles_i, tiles_j) == (12, 12) and nb == 2
    t = terrain(hip, g, arrays)
    ref = reference(g, arrays, obs, max_dist=4000.0)
    hist = vr.histogram(ref[0])
    assert min(hist) > 10000
    check(run(t, obs, mask.shape, max_dist=4000.0), ref)


def test_more_observers_than_one_launch_holds(hip):
    """MAX_POS + 40 observers, five distinct ones tiled: a wrong chunk offset in any output shows."""
    g = cases.rough_terrain(20, 20, seed=5, offset=2, relief=900.0)
    arrays = cases.terrain_inputs(g)
    mask = arrays[4]
    mask[2:4, 5:11] = 0
    x, y, z = g["x"], g["y"], g["z"]
    five = np.array([[x[10], y[10], z[10, 10] + 2.0], [x[3], y[15], z[15, 3] + 8.0], [x[17], y[4], z[4, 17] + 1.0],
                     [x[9] + 5.0, y[9] + 5.0, z.max() + 100.0], [x[0] - 100.0, y[19] - 60.0, z.min() + 20.0]], np.float32)
    codes5, _, cells5, _ = reference(g, arrays, five)
    assert len({c.tobytes() for c in codes5}) == 5 and len(set(cells5.tolist())) == 5
    n = MAX_POS + 40
    idx = np.arange(n) % 5
    obs = np.ascontiguousarray(five[idx])
    times = np.bincount(idx, minlength=5)
    seen_ref = np.where(mask == 1, ((codes5 == 0) * times[:, None, None]).sum(axis=0), -1).astype(np.int32)
    rays_ref = int((((codes5 == 0) | (codes5 == 2)).sum(axis=(1, 2)) * times).sum())
    t = terrain(hip, g, arrays)
    vis, seen, cells, st = run(t, obs, mask.shape)
    assert np.array_equal(cells, cells5[idx])
    assert np.array_equal(seen, seen_ref)
    assert np.array_equal(vis[:5], codes5) and np.array_equal(vis[MAX_POS - 3:MAX_POS + 2], codes5[idx[MAX_POS - 3:MAX_POS + 2]])
    assert np.array_equal(vis, codes5[idx])
    assert st["num_rays"] == rays_ref


def test_scratch_does_not_grow_with_the_observers(small):
    g, arrays, obs, t, refs = small
    shape = arrays[4].shape
    _, _, _, st1 = run(t, obs[:1].copy(), shape)
    many = np.ascontiguousarray(np.tile(obs, (50, 1)))
    _, seen, _, st2 = run(t, many, shape)
    assert st1["scratch_bytes"] == st2["scratch_bytes"]
    assert np.array_equal(seen, np.where(arrays[4] == 1, refs[(True, None)][1] * 50, -1))
