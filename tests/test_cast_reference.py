"""The CPU yardstick of Terrain.cast (tests/cast_reference.py) held to what is already trusted: the oracle's tree against its
brute-force mode on seeded ray sets with pinned hit counts -- so that the sets the GPU tests share cannot go trivial -- and
the contract's edges: an origin on a DEM vertex, a degenerate segment, a segment that ends on a vertex, and one piece of
plain geometry."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import cast_reference as cr
from tests import viewshed_reference as vr
from tests.test_viewshed_reference import fixture, near_observers

N = 4099
MAX_DIST = 3000.0
SHORT_DIST = 600.0
SEED_RAYS, SEED_SEGMENTS = 7, 11
# from this reference, with the tree equal to brute force in every case
HITS = {MAX_DIST: 899, SHORT_DIST: 644}                  # of the 4099 random rays
BLOCKED, FREE, DEGENERATE = 3182, 913, 4                 # of the 4099 segments between lifted vertices


@pytest.fixture(scope="module")
def small():
    g, *_ = fixture()
    return g, orc.Scene(g["vert_grid"], 40, 40)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(cr.words(a[1]), cr.words(b[1])) and
            np.array_equal(cr.words(a[2]), cr.words(b[2])) and a[3] == b[3])


def consistent(occ, dist, point):
    assert occ.dtype == np.uint8 and dist.dtype == np.float32 and point.dtype == np.float32
    assert np.array_equal(occ.astype(bool), ~np.isnan(dist))
    assert np.array_equal(np.isnan(point).all(axis=-1), np.isnan(dist)) and np.array_equal(np.isnan(point).any(axis=-1), np.isnan(dist))
    assert (cr.words(dist[np.isnan(dist)]) == 0x7fc00000).all()


@pytest.mark.parametrize("max_dist", (MAX_DIST, SHORT_DIST))
def test_random_rays_tree_equals_brute_force_and_hits_are_pinned(small, max_dist):
    g, scene = small
    org, dirs = cr.random_rays(g, N, SEED_RAYS)
    assert org.dtype == np.float32 and dirs.dtype == np.float32
    assert float(np.abs((dirs.astype(np.float64) ** 2).sum(axis=1) - 1.0).max()) <= 1e-6
    a = cr.cast(g["vert_grid"], 40, 40, org, directions=dirs, max_dist=max_dist, scene=scene)
    b = cr.cast(g["vert_grid"], 40, 40, org, directions=dirs, max_dist=max_dist, scene=scene, mode=orc.MODE_BRUTE)
    assert same(a, b)
    occ, dist, point, rays = a
    consistent(occ, dist, point)
    assert rays == N and int(occ.sum()) == HITS[max_dist]
    assert (dist[occ == 1] <= np.float32(max_dist)).all() and (dist[occ == 1] >= 0).all()


def test_random_segments_tree_equals_brute_force_and_classes_are_pinned(small):
    g, scene = small
    org, tgt = cr.random_segments(g["vert_grid"], 40, 40, N, SEED_SEGMENTS)
    a = cr.cast(g["vert_grid"], 40, 40, org, targets=tgt, scene=scene)
    b = cr.cast(g["vert_grid"], 40, 40, org, targets=tgt, scene=scene, mode=orc.MODE_BRUTE)
    assert same(a, b)
    occ, dist, point, rays = a
    consistent(occ, dist, point)
    degenerate = (org == tgt).all(axis=1)
    assert int(degenerate.sum()) == DEGENERATE and rays == N - DEGENERATE
    assert int(occ.sum()) == BLOCKED and int((occ == 0).sum()) - DEGENERATE == FREE
    # a degenerate segment: not occluded, no distance, no point, no ray
    assert (occ[degenerate] == 0).all() and np.isnan(dist[degenerate]).all() and np.isnan(point[degenerate]).all()
    # a hit lies within the segment
    mag = np.linalg.norm((tgt - org).astype(np.float64), axis=1)
    assert (dist[occ == 1] <= mag[occ == 1] * (1 + 1e-6)).all()


def test_origin_on_a_vertex_gives_distance_plus_zero(small):
    """The origin lies on the surface: the triangles around it accept T = +0 and T = -0 in every direction, and the clause
    writes +0.0."""
    g, scene = small
    v = vr.vertices(g["vert_grid"], 40, 40)[21, 13]
    _, dirs = cr.random_rays(g, 257, 3)
    org = np.ascontiguousarray(np.broadcast_to(v, dirs.shape))
    occ, dist, point, rays = cr.cast(g["vert_grid"], 40, 40, org, directions=dirs, max_dist=MAX_DIST, scene=scene)
    assert rays == 257 and (occ == 1).all()
    assert (cr.words(dist) == 0).all()                       # +0.0, never -0.0
    assert np.array_equal(point, org)
    # the same as segments towards far targets
    occ, dist, point, rays = cr.cast(g["vert_grid"], 40, 40, org, targets=org + dirs * np.float32(500.0), scene=scene)
    assert rays == 257 and (occ == 1).all() and (cr.words(dist) == 0).all() and np.array_equal(point, org)


def test_degenerate_segments_are_not_rays(small):
    g, scene = small
    obs = near_observers(g)
    org = np.ascontiguousarray(np.vstack([obs, obs[:2]]))
    tgt = org.copy()
    tgt[5] = obs[2]                                          # one real segment among six degenerate ones
    occ, dist, point, rays = cr.cast(g["vert_grid"], 40, 40, org, targets=tgt, scene=scene)
    assert rays == 1
    assert (occ[[0, 1, 2, 3, 4, 6]] == 0).all() and np.isnan(dist[[0, 1, 2, 3, 4, 6]]).all() and np.isnan(point[[0, 1, 2, 3, 4, 6]]).all()
    assert (cr.words(dist[[0, 1, 2, 3, 4, 6]]) == 0x7fc00000).all()


def test_segment_that_ends_on_a_vertex(small):
    """tfar is the distance to the target, and the target lies on the surface: whether the triangles around the vertex are
    accepted at t = tfar is the intersector's rounding -- the tree and brute force agree on it, and a hit is at the
    segment's end to 4 ulp.  Two metres short of the vertex the same segments are free."""
    g, scene = small
    verts = vr.vertices(g["vert_grid"], 40, 40)
    v = verts[21, 13]
    obs = near_observers(g)
    org = np.ascontiguousarray(obs[[0, 2]])                  # the summit and high above the middle: both see the vertex's surroundings
    tgt = np.ascontiguousarray(np.broadcast_to(v, org.shape))
    a = cr.cast(g["vert_grid"], 40, 40, org, targets=tgt, scene=scene)
    b = cr.cast(g["vert_grid"], 40, 40, org, targets=tgt, scene=scene, mode=orc.MODE_BRUTE)
    assert same(a, b) and a[3] == 2
    mag = np.linalg.norm((tgt - org).astype(np.float64), axis=1)
    print("occluded %r, dist %r, |target - origin| %r" % (a[0].tolist(), a[1].tolist(), mag.tolist()))
    for k in range(2):
        if a[0][k]:
            assert abs(float(a[1][k]) - mag[k]) <= 4 * np.spacing(np.float32(mag[k]))
    # the vertical one ends on the surface or an ulp short of it: from straight above the hit, if any, is at the end
    up = np.ascontiguousarray((v + np.array([0.0, 0.0, 500.0], np.float32))[None, :])
    occ, dist, _, _ = cr.cast(g["vert_grid"], 40, 40, up, targets=v[None, :], scene=scene)
    if occ[0]:
        assert abs(float(dist[0]) - 500.0) <= 4 * np.spacing(np.float32(500.0))
    short = cr.cast(g["vert_grid"], 40, 40, up, targets=(v + np.array([0.0, 0.0, 2.0], np.float32))[None, :], scene=scene)
    assert short[0][0] == 0 and np.isnan(short[1][0])


def test_vertical_ray_is_the_height_above_the_surface(small):
    """Straight down from the observer high above the middle: the distance is its height above the triangle below it -- the
    quad's triangles are (i, j), (i, j + 1), (i + 1, j) and (i, j + 1), (i + 1, j + 1), (i + 1, j) -- in float64.  The float32
    distance is T / den of sums of a few rounded products without cancellation (a vertical ray, a mild slope): 4 ulp."""
    g, scene = small
    x, y, z = g["x"].astype(np.float64), g["y"].astype(np.float64), g["z"].astype(np.float64)
    o = near_observers(g)[2]
    px, py, pz = (float(v) for v in o)
    j = int(np.searchsorted(x, px, "right") - 1)
    i = int(np.searchsorted(-y, -py, "right") - 1)              # y descends with the row
    u, v = (px - x[j]) / (x[j + 1] - x[j]), (y[i] - py) / (y[i] - y[i + 1])
    assert 0.0 < u < 1.0 and 0.0 < v < 1.0
    if u + v <= 1.0:
        surf = z[i, j] + u * (z[i, j + 1] - z[i, j]) + v * (z[i + 1, j] - z[i, j])
    else:
        surf = z[i + 1, j + 1] + (1.0 - u) * (z[i + 1, j] - z[i + 1, j + 1]) + (1.0 - v) * (z[i, j + 1] - z[i + 1, j + 1])
    height = pz - surf
    down = np.array([[0.0, 0.0, -1.0]], np.float32)
    occ, dist, point, _ = cr.cast(g["vert_grid"], 40, 40, o[None, :], directions=down, max_dist=MAX_DIST, scene=scene)
    print("height above the surface %.6f, distance %r" % (height, float(dist[0])))
    assert height == pytest.approx(1703.2, abs=0.05)
    assert occ[0] == 1 and abs(float(dist[0]) - height) <= 4 * np.spacing(np.float32(height))
    assert abs(float(point[0, 2]) - surf) <= 4 * np.spacing(np.float32(height))
    assert point[0, 0] == o[0] and point[0, 1] == o[1]
    # the same ray as a segment to a point below the surface stops at the same distance; one that ends above it is free
    below = (o + np.array([0.0, 0.0, -2000.0], np.float32))[None, :]
    seg = cr.cast(g["vert_grid"], 40, 40, o[None, :], targets=below, scene=scene)
    assert seg[0][0] == 1 and np.array_equal(cr.words(seg[1]), cr.words(dist))
    above = (o + np.array([0.0, 0.0, -1700.0], np.float32))[None, :]
    assert cr.cast(g["vert_grid"], 40, 40, o[None, :], targets=above, scene=scene)[0][0] == 0
    # too short a ray reaches nothing
    assert cr.cast(g["vert_grid"], 40, 40, o[None, :], directions=down, max_dist=1700.0, scene=scene)[0][0] == 0
