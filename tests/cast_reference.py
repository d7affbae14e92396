"""CPU yardstick of Terrain.cast (clause 21): the rays of the caller restated in NumPy float32 -- every
product, sum, square root and quotient an array operation of its own, so each is rounded on its own -- and traced by the
oracle with a tfar per ray (oracle.Scene.occluded: is any triangle accepted; oracle.Scene.closest: the minimum t over all
accepted triangles).  The GPU tests hold the kernels to these words bit for bit."""
import numpy as np

from oracle import oracle as orc

F = np.float32


def rays(origins, directions=None, targets=None, max_dist=None):
    """(origins f32[N][3], dirs f32[N][3], tfar f32[N], live bool[N]) of the clause's steps 1 and 2.  A segment whose target
    is its origin is not live: it gives no ray (its direction and tfar here are placeholders)."""
    origins = np.ascontiguousarray(origins, F).reshape(-1, 3)
    n = origins.shape[0]
    assert (directions is None) != (targets is None)
    if directions is not None:
        dirs = np.ascontiguousarray(directions, F).reshape(-1, 3)
        assert dirs.shape == (n, 3) and max_dist is not None
        return origins, dirs, np.full(n, F(max_dist), F), np.ones(n, bool)
    assert max_dist is None
    targets = np.ascontiguousarray(targets, F).reshape(-1, 3)
    assert targets.shape == (n, 3)
    d = targets - origins
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    mag = np.sqrt((dx * dx + dy * dy) + dz * dz)
    live = mag > F(0.0)
    with np.errstate(all="ignore"):
        u = d / mag[:, None]
    for v in (d, mag, u):
        assert v.dtype == F
    u[~live] = F(0.0)
    u[~live, 2] = F(1.0)
    return origins, u, np.where(live, mag, F(1.0)).astype(F), live


def cast(vert_grid, dem_dim_0, dem_dim_1, origins, directions=None, targets=None, max_dist=None, mode=orc.MODE_BVH,
         scene=None):
    """(occluded u8[N], dist f32[N], point f32[N][3], rays traced)."""
    if scene is None:
        scene = orc.Scene(vert_grid, dem_dim_0, dem_dim_1)
    org, dirs, tfar, live = rays(origins, directions, targets, max_dist)
    n = org.shape[0]
    occ = np.zeros(n, bool)
    hit = np.zeros(n, bool)
    t = np.zeros(n, F)
    if live.any():
        occ[live] = scene.occluded(org[live], dirs[live], tfar[live], mode=mode)                  # step 3
        hit[live], t[live] = scene.closest(org[live], dirs[live], tfar[live], mode=mode)          # step 4
    assert t.dtype == F
    t = np.where(t == F(0.0), F(0.0), t)                                        # a zero minimum is written as +0.0
    dist = np.where(hit, t, F(np.nan)).astype(F)
    with np.errstate(invalid="ignore"):
        prod = dirs * dist[:, None]                                             # step 5: a product ...
        point = org + prod                                                      # ... then a sum
    assert prod.dtype == F and point.dtype == F
    point[~hit] = F(np.nan)
    # hz_tri_hit_t accepts exactly what hz_tri_hit accepts: the any-hit answer is the closest-hit one
    assert np.array_equal(occ, hit)
    return occ.astype(np.uint8), dist, point, int(live.sum())


def words(a):
    """The 32-bit words of a float32 array: equality of all words is equality of all values, NaN positions included."""
    a = np.ascontiguousarray(a)
    assert a.dtype == F
    return a.view(np.uint32)


def random_rays(g, n, seed):
    """n rays with origins uniform in the terrain's box grown by 200 m sideways, from 50 m below its lowest point to 300 m
    above its highest, and isotropic unit directions, all float32."""
    rng = np.random.default_rng(seed)
    x, y, z = g["x"].astype(np.float64), g["y"].astype(np.float64), g["z"].astype(np.float64)
    lo = np.array([x.min() - 200.0, y.min() - 200.0, z.min() - 50.0])
    hi = np.array([x.max() + 200.0, y.max() + 200.0, z.max() + 300.0])
    org = (lo + rng.random((n, 3)) * (hi - lo)).astype(F)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.ascontiguousarray(org), np.ascontiguousarray(v.astype(F))


def random_segments(vert_grid, dem_dim_0, dem_dim_1, n, seed, lift=2.0):
    """n segments between random pairs of DEM vertices lifted by `lift` m; a pair of one vertex with itself is degenerate."""
    rng = np.random.default_rng(seed)
    v = np.ascontiguousarray(vert_grid, F)[:3 * dem_dim_0 * dem_dim_1].reshape(-1, 3)
    up = np.array([0.0, 0.0, lift], F)
    a, b = rng.integers(0, v.shape[0], n), rng.integers(0, v.shape[0], n)
    return np.ascontiguousarray(v[a] + up), np.ascontiguousarray(v[b] + up)
