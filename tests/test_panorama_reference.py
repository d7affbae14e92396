"""The CPU yardstick of Terrain.panorama (tests/panorama_reference.py) held to what is already trusted: the oracle's tree
against its brute-force mode, pinned hit counts so that the fixture the GPU tests share cannot go trivial, the contract's
edge (an observer on a DEM vertex) and one piece of plain geometry."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import panorama_reference as pr
from tests import viewshed_reference as vr
from tests.test_viewshed_reference import fixture, near_observers

MAX_DIST = 3000.0
SHORT_DIST = 600.0
GRIDS = ((45, 21), (13, 5))            # (A, E)

# hits per observer (summit, pit, high above the middle, outside the DEM, near a corner, on a vertex), from this reference
# with the tree equal to brute force in every case
HITS = {
    (45, 21, MAX_DIST): [163, 775, 176, 19, 504, 945],
    (13, 5, MAX_DIST): [17, 52, 13, 2, 33, 65],
    (45, 21, SHORT_DIST): [116, 774, 0, 0, 504, 945],
    (13, 5, SHORT_DIST): [14, 52, 0, 0, 33, 65],
}


def six_observers(g):
    """The five near observers of the viewshed tests and a sixth exactly on DEM vertex (21, 13)."""
    on_vertex = vr.vertices(g["vert_grid"], 40, 40)[21, 13]
    return np.ascontiguousarray(np.vstack([near_observers(g), on_vertex[None, :]]), np.float32)


def angles(num_azim, num_elev):
    azim = np.linspace(0.0, 2.0 * np.pi, num_azim, endpoint=False).astype(np.float32)
    elev = np.linspace(-np.pi / 2, np.pi / 2, num_elev).astype(np.float32)
    return azim, elev


@pytest.fixture(scope="module")
def small():
    g, *_ = fixture()
    return g, six_observers(g), orc.Scene(g["vert_grid"], 40, 40)


def reference(small, grid, max_dist, **kw):
    g, obs, scene = small
    azim, elev = angles(*grid)
    return pr.panorama(g["vert_grid"], 40, 40, obs, azim, elev, max_dist, scene=scene, **kw)


@pytest.mark.parametrize("max_dist", (MAX_DIST, SHORT_DIST))
@pytest.mark.parametrize("grid", GRIDS)
def test_tree_equals_brute_force_and_hits_are_pinned(small, grid, max_dist):
    a = reference(small, grid, max_dist)
    b = reference(small, grid, max_dist, mode=orc.MODE_BRUTE)
    assert np.array_equal(pr.words(a[0]), pr.words(b[0]))
    assert np.array_equal(pr.words(a[1]), pr.words(b[1]))
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] == 6 * grid[0] * grid[1]
    dist, point, hits, rays = a
    assert dist.dtype == np.float32 and point.dtype == np.float32 and hits.dtype == np.int64
    assert dist.shape == (6, grid[1], grid[0]) and point.shape == dist.shape + (3,)
    assert hits.tolist() == HITS[grid + (max_dist,)]
    assert np.array_equal(hits, (~np.isnan(dist)).sum(axis=(1, 2)))
    # a pixel has a point exactly where it has a distance, and every distance is within the ray
    assert np.array_equal(np.isnan(point).all(axis=-1), np.isnan(dist)) and np.array_equal(np.isnan(point).any(axis=-1), np.isnan(dist))
    assert (dist[~np.isnan(dist)] <= np.float32(max_dist)).all() and (dist[~np.isnan(dist)] >= 0).all()


def test_short_rays_leave_two_observers_without_a_hit(small):
    """max_dist = 600: the observer high above the middle and the one outside the DEM see whole images of NaN."""
    dist, point, hits, _ = reference(small, (45, 21), SHORT_DIST)
    assert hits[2] == 0 and hits[3] == 0
    assert np.isnan(dist[2:4]).all() and np.isnan(point[2:4]).all()
    assert (pr.words(dist[2:4]) == 0x7fc00000).all()


def test_observer_on_a_vertex_hits_every_pixel_at_distance_zero(small):
    """The contract's edge: the origin lies on the surface, the triangle test accepts T = 0 in every direction."""
    g, obs, _ = small
    for grid in GRIDS:
        dist, point, hits, _ = reference(small, grid, MAX_DIST)
        assert hits[5] == grid[0] * grid[1]
        assert (dist[5] == 0.0).all()
        assert np.array_equal(point[5], np.broadcast_to(obs[5], point[5].shape))


def test_straight_down_pixel_is_the_height_above_the_surface(small):
    """elev = -pi/2 of the observer high above the middle: the distance is its height above the triangle below it -- the
    quad's triangles are (i, j), (i, j + 1), (i + 1, j) and (i, j + 1), (i + 1, j + 1), (i + 1, j) -- in float64.  The float32
    distance is T / den of sums of a few rounded products without cancellation (a vertical ray, a mild slope): 4 ulp."""
    g, obs, _ = small
    x, y, z = g["x"].astype(np.float64), g["y"].astype(np.float64), g["z"].astype(np.float64)
    px, py, pz = (float(v) for v in obs[2])
    j = int(np.searchsorted(x, px, "right") - 1)
    i = int(np.searchsorted(-y, -py, "right") - 1)              # y descends with the row
    u, v = (px - x[j]) / (x[j + 1] - x[j]), (y[i] - py) / (y[i] - y[i + 1])
    assert 0.0 < u < 1.0 and 0.0 < v < 1.0
    if u + v <= 1.0:
        surf = z[i, j] + u * (z[i, j + 1] - z[i, j]) + v * (z[i + 1, j] - z[i, j])
    else:
        surf = z[i + 1, j + 1] + (1.0 - u) * (z[i + 1, j] - z[i + 1, j + 1]) + (1.0 - v) * (z[i, j + 1] - z[i + 1, j + 1])
    height = pz - surf
    dist, point, _, _ = reference(small, (45, 21), MAX_DIST)
    down = dist[2, 0, :]
    print("height above the surface %.6f, straight-down pixels %r ... %r" % (height, float(down.min()), float(down.max())))
    assert height == pytest.approx(1703.2, abs=0.05)
    assert np.abs(down.astype(np.float64) - height).max() <= 4 * np.spacing(np.float32(height))
    assert np.abs(point[2, 0, :, 2].astype(np.float64) - surf).max() <= 4 * np.spacing(np.float32(height))


def test_frames_rotate_the_image(small):
    """A frame turned by a quarter about the vertical shifts the azimuths: north = east of the default frame makes azimuth a
    look where azimuth a + 90 degrees looked (45 azimuths do not hold a quarter turn: 16 do).  The float32 azimuths are
    off their exact values by up to half an ulp of 2 pi (2.4e-7), so the two sets of directions agree to 1e-6."""
    g, obs, scene = small
    azim, elev = angles(16, 5)
    north = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (6, 1))
    norm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (6, 1))
    turned = pr.rays(obs, azim, elev, north, norm)
    assert turned.shape == (6, 5, 16, 3)
    assert np.abs(turned - np.roll(pr.rays(obs, azim, elev), -4, axis=2)).max() <= 1e-6
    # azimuth 0 of the default frame looks north, azimuth 4 of 16 east; elevation index 2 of 5 is level
    plain_rays = pr.rays(obs, azim, elev)
    assert np.abs(plain_rays[0, 2, 0] - [0.0, 1.0, 0.0]).max() <= 1e-6 and np.abs(plain_rays[0, 2, 4] - [1.0, 0.0, 0.0]).max() <= 1e-6
    assert np.abs(plain_rays[0, 4, 0] - [0.0, 0.0, 1.0]).max() <= 1e-6
    plain = pr.panorama(g["vert_grid"], 40, 40, obs, azim, elev, MAX_DIST, scene=scene)
    # the default frame given explicitly is the default left out, word for word
    north = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (6, 1))
    same = pr.panorama(g["vert_grid"], 40, 40, obs, azim, elev, MAX_DIST, north, norm, scene=scene)
    assert np.array_equal(pr.words(same[0]), pr.words(plain[0])) and np.array_equal(pr.words(same[1]), pr.words(plain[1]))
