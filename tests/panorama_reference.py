"""CPU yardstick of Terrain.panorama (clause 20): the rays of every observer's image restated in NumPy
float32 -- every product and sum an array operation of its own, so each is rounded on its own -- and traced by the oracle
(oracle.Scene.closest: the minimum t over all accepted triangles).  The four trig tables are restated here, not taken from
the library.  The GPU tests hold the kernel to these words bit for bit."""
import numpy as np

from oracle import oracle as orc

F = np.float32


def tables(azim, elev):
    """(azim_sin, azim_cos, elev_sin, elev_cos): float64 sin / cos of the float32 angles, rounded to float32 once."""
    azim = np.asarray(azim, F).astype(np.float64)
    elev = np.asarray(elev, F).astype(np.float64)
    return np.sin(azim).astype(F), np.cos(azim).astype(F), np.sin(elev).astype(F), np.cos(elev).astype(F)


def rays(observers, azim, elev, vec_north=None, vec_norm=None):
    """The ray directions f32[S][E][A][3] of the clause (steps 1 - 3)."""
    observers = np.ascontiguousarray(observers, F).reshape(-1, 3)
    n = observers.shape[0]
    if vec_north is None:
        assert vec_norm is None
        north = np.tile(np.array([0.0, 1.0, 0.0], F), (n, 1))
        norm = np.tile(np.array([0.0, 0.0, 1.0], F), (n, 1))
    else:
        north, norm = np.ascontiguousarray(vec_north, F), np.ascontiguousarray(vec_norm, F)
        assert north.shape == (n, 3) and norm.shape == (n, 3)
    azim_sin, azim_cos, elev_sin, elev_cos = tables(azim, elev)
    east = np.stack([north[:, 1] * norm[:, 2] - north[:, 2] * norm[:, 1],
                     north[:, 2] * norm[:, 0] - north[:, 0] * norm[:, 2],
                     north[:, 0] * norm[:, 1] - north[:, 1] * norm[:, 0]], axis=-1)
    rx = elev_cos[:, None] * azim_sin[None, :]
    ry = elev_cos[:, None] * azim_cos[None, :]
    rz = np.broadcast_to(elev_sin[:, None], rx.shape)
    a = east[:, None, None, :] * rx[None, :, :, None]
    b = north[:, None, None, :] * ry[None, :, :, None]
    c = norm[:, None, None, :] * rz[None, :, :, None]
    dirs = (a + b) + c
    for v in (east, rx, ry, a, b, c, dirs):
        assert v.dtype == F
    return dirs


def panorama(vert_grid, dem_dim_0, dem_dim_1, observers, azim, elev, max_dist, vec_north=None, vec_norm=None,
             mode=orc.MODE_BVH, scene=None):
    """(dist f32[S][E][A], point f32[S][E][A][3], hits i64[S], rays) for observers f32[S][3]."""
    if scene is None:
        scene = orc.Scene(vert_grid, dem_dim_0, dem_dim_1)
    observers = np.ascontiguousarray(observers, F).reshape(-1, 3)
    dirs = rays(observers, azim, elev, vec_north, vec_norm)
    org = np.ascontiguousarray(np.broadcast_to(observers[:, None, None, :], dirs.shape))
    hit, t = scene.closest(org.reshape(-1, 3), dirs.reshape(-1, 3), F(max_dist), mode=mode)
    hit = hit.reshape(dirs.shape[:3])
    t = t.reshape(dirs.shape[:3])
    assert t.dtype == F
    # step 4: a zero minimum is written as +0.0 -- around an origin on the surface triangles are accepted with T = +0 and
    # T = -0, and which of the two equal values a minimum keeps depends on the order they are met in
    t = np.where(t == F(0.0), F(0.0), t)
    dist = np.where(hit, t, F(np.nan)).astype(F)
    with np.errstate(invalid="ignore"):
        prod = dirs * dist[..., None]                                           # step 5: a product ...
        point = org + prod                                                      # ... then a sum
    assert prod.dtype == F and point.dtype == F
    point[~hit] = F(np.nan)
    hits = hit.sum(axis=(1, 2)).astype(np.int64)
    return dist, point, hits, int(hit.size)


def words(a):
    """The 32-bit words of a float32 array: equality of all words is equality of all values, NaN positions included."""
    a = np.ascontiguousarray(a)
    assert a.dtype == F
    return a.view(np.uint32)
