"""Terrain.panorama on the GPU: every case word for word (uint32 views, NaN positions included) against the CPU yardstick
(tests/panorama_reference.py: the NumPy float32 rays and the oracle's closest hits) -- distances, hit points, hit counts and
the number of rays."""
import itertools

import numpy as np
import pytest

from tests import cases
from tests import horidist_reference as hd
from tests import panorama_reference as pr
from tests.test_panorama_reference import HITS, MAX_DIST, SHORT_DIST, angles, six_observers
from tests.test_viewshed_reference import fixture

pytestmark = pytest.mark.gpu

GRIDS = ((45, 21), (13, 5), (1, 1), (64, 8), (65, 9))          # (A, E): partial tiles on both axes, one pixel, exact tiles, one over
JUNK = np.float32(-77.25)


class knob:
    """hz_debug_set(key, value) for the block, the default restored afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key.encode(), value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, -1))
        return False


def terrain(hip, g, arrays):
    vec_tilt, vec_norm, enl, elev, mask = arrays
    t = hip.shadow.Terrain()
    t.initialise(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_tilt, vec_norm, enl, elev, mask)
    return t


def tilted_frames(n):
    """Unit (north, norm) per observer, each observer's tilted and turned differently (as on a curved DEM, exaggerated)."""
    k = np.arange(n, dtype=np.float64)
    ax, ay, turn = 0.05 * (k - 2.0), 0.03 * (3.0 - k), 0.4 * k - 1.0
    norm = np.stack([np.sin(ay), -np.sin(ax) * np.cos(ay), np.cos(ax) * np.cos(ay)], axis=1)
    north0 = np.array([0.0, 1.0, 0.0])
    north = north0[None, :] - (norm * north0).sum(axis=1, keepdims=True) * norm
    north /= np.linalg.norm(north, axis=1, keepdims=True)
    east = np.cross(north, norm)
    north = np.cos(turn)[:, None] * north + np.sin(turn)[:, None] * east
    return np.ascontiguousarray(north, np.float32), np.ascontiguousarray(norm, np.float32)


def run(t, obs, azim, elev, max_dist, want=(True, True, True), **kw):
    """(dist, point, hits, stats) into NumPy buffers filled with junk; None for an output not asked for."""
    n, shape = obs.shape[0], (obs.shape[0], elev.shape[0], azim.shape[0])
    dist = np.full(shape, JUNK, np.float32) if want[0] else None
    point = np.full(shape + (3,), JUNK, np.float32) if want[1] else None
    hits = np.full(n, -77, np.int64) if want[2] else None
    t.panorama(obs, azim, elev, max_dist, dist=dist, point=point, hits=hits, **kw)
    return dist, point, hits, dict(t.last_stats)


def check(got, ref):
    dist, point, hits, st = got
    dist_ref, point_ref, hits_ref, rays = ref
    print("rays %d / %d, dist words differing %s, point words differing %s, hits differing %s" % (
        st["num_rays"], rays, None if dist is None else int((pr.words(dist) != pr.words(dist_ref)).sum()),
        None if point is None else int((pr.words(point) != pr.words(point_ref)).sum()),
        None if hits is None else int((hits != hits_ref).sum())))
    for name, a, b in (("dist", dist, dist_ref), ("point", point, point_ref)):
        if a is not None and a.shape == b.shape:
            for idx in np.argwhere(pr.words(a) != pr.words(b))[:8]:
                print("  %s%s: %r (0x%08x), reference %r (0x%08x)" % (name, tuple(int(i) for i in idx), float(a[tuple(idx)]),
                                                                    int(pr.words(a)[tuple(idx)]), float(b[tuple(idx)]), int(pr.words(b)[tuple(idx)])))
    if dist is not None:
        assert dist.shape == dist_ref.shape and np.array_equal(pr.words(dist), pr.words(dist_ref))
    if point is not None:
        assert point.shape == point_ref.shape and np.array_equal(pr.words(point), pr.words(point_ref))
    if hits is not None:
        assert hits.dtype == np.int64 and np.array_equal(hits, hits_ref)
    assert st["num_rays"] == rays


class Small:
    """The 40 x 40 fixture of the CPU tests, its six observers, a Terrain, and the references, each computed once."""

    def __init__(self, hip):
        from oracle import oracle as orc
        self.g, *self.arrays = fixture()
        self.obs = six_observers(self.g)
        self.t = terrain(hip, self.g, self.arrays)
        self.scene = orc.Scene(self.g["vert_grid"], 40, 40)
        self.frames = tilted_frames(6)
        self.refs = {}

    def ref(self, grid, max_dist, tilted=False, first=0, count=6):
        key = (grid, max_dist, tilted, first, count)
        if key not in self.refs:
            azim, elev = angles(*grid)
            fr = tuple(f[first:first + count] for f in self.frames) if tilted else (None, None)
            r = pr.panorama(self.g["vert_grid"], 40, 40, self.obs[first:first + count], azim, elev, max_dist, *fr, scene=self.scene)
            for a in r[:3]:
                a.setflags(write=False)
            self.refs[key] = r
        return self.refs[key]


@pytest.fixture(scope="module")
def small(hip):
    return Small(hip)


@pytest.mark.parametrize("max_dist", (MAX_DIST, SHORT_DIST))
@pytest.mark.parametrize("grid", GRIDS)
def test_six_observers(small, grid, max_dist):
    ref = small.ref(grid, max_dist)
    if grid + (max_dist,) in HITS:
        assert ref[2].tolist() == HITS[grid + (max_dist,)]
    if max_dist == SHORT_DIST:
        assert ref[2][2] == 0 and ref[2][3] == 0              # whole images of NaN
    azim, elev = angles(*grid)
    check(run(small.t, small.obs, azim, elev, max_dist), ref)


@pytest.mark.parametrize("grid", GRIDS)
def test_one_observer(small, grid):
    azim, elev = angles(*grid)
    for s in (0, 3, 5):
        check(run(small.t, small.obs[s:s + 1], azim, elev, MAX_DIST), small.ref(grid, MAX_DIST, first=s, count=1))


@pytest.mark.parametrize("grid", ((45, 21), (13, 5)))
def test_tilted_frames_per_observer(small, grid):
    azim, elev = angles(*grid)
    north, norm = small.frames
    assert not np.array_equal(north[0], north[1]) and not np.array_equal(norm[0], norm[1])
    ref = small.ref(grid, MAX_DIST, tilted=True)
    assert not np.array_equal(pr.words(ref[0]), pr.words(small.ref(grid, MAX_DIST)[0]))
    check(run(small.t, small.obs, azim, elev, MAX_DIST, vec_north=north, vec_norm=norm), ref)
    # one observer of the six with its own frame
    check(run(small.t, small.obs[4:5], azim, elev, MAX_DIST, vec_north=north[4:5], vec_norm=norm[4:5]),
          small.ref(grid, MAX_DIST, tilted=True, first=4, count=1))


def test_default_frame_given_explicitly(small):
    azim, elev = angles(45, 21)
    north = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (6, 1))
    norm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (6, 1))
    check(run(small.t, small.obs, azim, elev, MAX_DIST, vec_north=north, vec_norm=norm), small.ref((45, 21), MAX_DIST))


def test_unordered_angles(small):
    """No order or spacing of the angles is required: a shuffled image is the shuffled reference."""
    azim, elev = angles(45, 21)
    rng = np.random.default_rng(5)
    pa, pe = rng.permutation(45), rng.permutation(21)
    ref = small.ref((45, 21), MAX_DIST)
    want = (np.ascontiguousarray(ref[0][:, pe][:, :, pa]), np.ascontiguousarray(ref[1][:, pe][:, :, pa]), ref[2], ref[3])
    check(run(small.t, small.obs, np.ascontiguousarray(azim[pa]), np.ascontiguousarray(elev[pe]), MAX_DIST), want)


def test_every_subset_of_the_outputs_in_hbm_and_numpy(small):
    """The words do not depend on which outputs are asked for, nor on where they and the observers live."""
    torch = pytest.importorskip("torch")
    grid = (13, 5)
    azim, elev = angles(*grid)
    t, obs = small.t, small.obs
    ref = small.ref(grid, SHORT_DIST)
    dev = "cuda:%d" % t.device
    d_obs = torch.from_numpy(obs).to(dev)
    shape = (6, 5, 13)
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            continue
        check(run(t, obs, azim, elev, SHORT_DIST, want), ref)
        dist = torch.full(shape, float(JUNK), dtype=torch.float32, device=dev) if want[0] else None
        point = torch.full(shape + (3,), float(JUNK), dtype=torch.float32, device=dev) if want[1] else None
        hits = torch.full((6,), -77, dtype=torch.int64, device=dev) if want[2] else None
        torch.cuda.synchronize()
        # observers in HBM with the outputs in HBM; observers on the host for the odd subsets
        t.panorama(d_obs if want[0] == want[1] else obs, azim, elev, SHORT_DIST, dist=dist, point=point, hits=hits)
        torch.cuda.synchronize()
        check(tuple(None if b is None else b.cpu().numpy() for b in (dist, point, hits)) + (dict(t.last_stats),), ref)
    # observers in HBM, outputs on the host; then one output on each side
    check(run(t, d_obs, azim, elev, SHORT_DIST), ref)
    dist = np.full(shape, JUNK, np.float32)
    point = torch.full(shape + (3,), float(JUNK), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t.panorama(obs, azim, elev, SHORT_DIST, dist=dist, point=point)
    torch.cuda.synchronize()
    check((dist, point.cpu().numpy(), None, dict(t.last_stats)), ref)


def test_chunks_of_observers_give_the_words_of_one_chunk(small):
    """`panorama_budget` cuts the observers into chunks of 1, of 4 with a short last chunk of 2, and (five observers) of 2
    with a short last chunk of 1; the staging reported does not grow with the number of observers."""
    torch = pytest.importorskip("torch")
    grid = (45, 21)
    azim, elev = angles(*grid)
    t, obs = small.t, small.obs
    ref6, ref5 = small.ref(grid, MAX_DIST), small.ref(grid, MAX_DIST, count=5)
    per_obs = 45 * 21 * 16                                    # dist and point staged
    tables = 2 * (45 + 21) * 4
    got = run(t, obs, azim, elev, MAX_DIST)
    check(got, ref6)
    assert got[3]["scratch_bytes"] == 6 * per_obs + tables + 6 * 12          # one chunk: everything staged at once
    for k, n, ref in ((1, 6, ref6), (4, 6, ref6), (2, 5, ref5), (2, 6, ref6)):
        with knob("panorama_budget", k * per_obs + 7):
            got = run(t, obs[:n], azim, elev, MAX_DIST)
        check(got, ref)
        assert got[3]["scratch_bytes"] == k * per_obs + tables + k * 12, (k, n)
    # dist alone is staged (4 bytes per pixel); point lies in HBM and is written in place, chunk after chunk
    dev = "cuda:%d" % t.device
    with knob("panorama_budget", 2 * 45 * 21 * 4):
        dist = np.full((6, 21, 45), JUNK, np.float32)
        point = torch.full((6, 21, 45, 3), float(JUNK), dtype=torch.float32, device=dev)
        hits = torch.full((6,), -77, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        north, norm = small.frames
        t.panorama(obs, azim, elev, MAX_DIST, dist=dist, point=point, hits=hits, vec_north=north, vec_norm=norm)
        torch.cuda.synchronize()
        st = dict(t.last_stats)
    check((dist, point.cpu().numpy(), hits.cpu().numpy(), st), small.ref(grid, MAX_DIST, tilted=True))
    assert st["scratch_bytes"] == 2 * 45 * 21 * 4 + tables + 2 * 36
    # nothing staged: the budget plays no part
    with knob("panorama_budget", 1):
        d_dist = torch.full((6, 21, 45), float(JUNK), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t.panorama(torch.from_numpy(obs).to(dev), azim, elev, MAX_DIST, dist=d_dist)
        torch.cuda.synchronize()
    check((d_dist.cpu().numpy(), None, None, dict(t.last_stats)), ref6)
    assert t.last_stats["scratch_bytes"] == tables


def test_traversal_order_does_not_matter(small):
    """The distance is the minimum over all accepted triangles: hz_closest's slot order gives the words of the front-to-back
    order."""
    for grid, max_dist, tilted in (((45, 21), MAX_DIST, False), ((65, 9), SHORT_DIST, False), ((45, 21), MAX_DIST, True)):
        azim, elev = angles(*grid)
        kw = dict(vec_north=small.frames[0], vec_norm=small.frames[1]) if tilted else {}
        for mode in (0, 1):
            with knob("panorama_traversal", mode):
                check(run(small.t, small.obs, azim, elev, max_dist, **kw), small.ref(grid, max_dist, tilted=tilted))


def test_deeper_tree(hip, small):
    """A non-square terrain whose tree is one level higher than the fixture's."""
    from oracle import oracle as orc
    g = cases.rough_terrain(96, 72, seed=17, offset=4, relief=1200.0)
    t = terrain(hip, g, cases.terrain_inputs(g))
    x, y, z = g["x"], g["y"], g["z"]
    hi = np.unravel_index(np.argmax(z), z.shape)
    obs = np.array([[x[hi[1]], y[hi[0]], z[hi] + 2.0], [x[30] + 11.0, y[50] - 4.0, z[50, 30] + 25.0]], np.float32)
    azim, elev = angles(45, 21)
    ref = pr.panorama(g["vert_grid"], 96, 72, obs, azim, elev, MAX_DIST, scene=orc.Scene(g["vert_grid"], 96, 72))
    assert 100 < ref[2][0] < 945 and 100 < ref[2][1] < 945, ref[2]
    got = run(t, obs, azim, elev, MAX_DIST)
    check(got, ref)
    run(small.t, small.obs[:1], azim, elev, MAX_DIST)
    print("tree heights", got[3]["bvh_height"], small.t.last_stats["bvh_height"])
    assert got[3]["bvh_height"] > small.t.last_stats["bvh_height"] >= 1


def test_horizon_distance_is_unchanged(hip, orc, small):
    """Its traversal moved to a header the panorama shares: the call still gives the reference's words."""
    kw = cases.grid_kwargs(small.g)
    par = dict(dist_search=2.0)
    hori, _ = orc.horizon_gridded(**kw, azim_num=24, **par)
    want = hd.horizon_distance(**kw, hori=hori, **par)
    assert 0.0 < float(np.isnan(want).mean()) < 0.5
    for mode in (1, 0):
        with knob("horidist_traversal", mode):
            got = hip.horizon.horizon_distance(**kw, hori=hori, **par)
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(hd.words(got), hd.words(want)), mode
