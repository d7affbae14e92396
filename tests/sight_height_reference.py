"""CPU yardstick of Terrain.sight_height (clause 19): the search of every (observer, cell) pair restated
in NumPy float32 -- every product, sum, square root and quotient an array operation of its own, so each is rounded on its
own -- with the rays traced by the oracle (oracle.Scene.occluded), round by round over the cells still searching: the top
of the table, its bottom, then one round per bisection step.  The GPU tests hold the kernel to these words bit for bit."""
import numpy as np

from oracle import oracle as orc
from tests.viewshed_reference import vertices

F = np.float32


class _Observer:
    """visible(k) of the clause for one observer over a flat list of cells; counts the rays it traces."""

    def __init__(self, scene, v, norm, heights, p, mode):
        self.scene, self.v, self.norm, self.heights, self.p, self.mode = scene, v, norm, heights, p, mode
        self.rays = 0

    def rays_to(self, cells, k):
        """(T_k, u, mag) of the cells `cells` for the table indices `k` (one per cell)."""
        h = self.heights[k]
        assert h.dtype == F
        lift = self.norm[cells] * h[:, None]
        target = self.v[cells] + lift
        d = self.p[None, :] - target
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        mag = np.sqrt((dx * dx + dy * dy) + dz * dz)
        u = d / mag[:, None]
        assert target.dtype == F and mag.dtype == F and u.dtype == F
        return target, u, mag

    def visible(self, cells, k):
        target, u, mag = self.rays_to(cells, k)
        vis = np.ones(cells.shape[0], bool)                 # !(mag > 0): visible, no ray
        ray = mag > F(0.0)
        n = int(ray.sum())
        if n:
            vis[ray] = ~self.scene.occluded(target[ray], u[ray], mag[ray], mode=self.mode)
        self.rays += n
        return vis


def _setup(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_norm, mask, observers, heights, scene):
    in0, in1 = mask.shape
    if scene is None:
        scene = orc.Scene(vert_grid, dem_dim_0, dem_dim_1)
    v = np.ascontiguousarray(vertices(vert_grid, dem_dim_0, dem_dim_1)[offset_0:offset_0 + in0, offset_1:offset_1 + in1]).reshape(-1, 3)
    norm = np.ascontiguousarray(vec_norm, F).reshape(-1, 3)
    observers = np.ascontiguousarray(observers, F).reshape(-1, 3)
    heights = np.ascontiguousarray(heights, F)
    assert heights.ndim == 1 and 1 <= heights.size <= 65535 and np.isfinite(heights).all()
    assert heights[0] >= F(0.005) and (heights[1:] > heights[:-1]).all()
    return scene, v, norm, observers, heights


def sight_height(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_norm, mask, observers, heights,
                 max_dist=None, mode=orc.MODE_BVH, scene=None):
    """(height f32[S][y][x], lowest f32[y][x], cells_reached i64[S], rays) for observers f32[S][3] and the table heights."""
    scene, v, norm, observers, heights = _setup(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_norm, mask,
                                                observers, heights, scene)
    n = heights.size
    on = (mask == 1).ravel()
    height = np.empty((observers.shape[0], on.size), F)
    rays = 0
    with np.errstate(all="ignore"):
        for s, p in enumerate(observers):
            ob = _Observer(scene, v, norm, heights, p, mode)
            res = np.full(on.size, np.nan, F)                                   # 1: masked
            todo = np.flatnonzero(on)
            if max_dist is not None:                                            # 2: out of range at the lowest target point
                _, _, mag0 = ob.rays_to(todo, np.zeros(todo.size, np.int64))
                far = mag0 > F(max_dist)
                res[todo[far]] = np.inf
                todo = todo[~far]
            top = ob.visible(todo, np.full(todo.size, n - 1, np.int64))         # 3: the top of the table
            res[todo[~top]] = np.inf
            todo = todo[top]
            if n == 1:                                                          # 4
                res[todo] = heights[0]
            else:
                bottom = ob.visible(todo, np.zeros(todo.size, np.int64))
                res[todo[bottom]] = heights[0]
                todo = todo[~bottom]
                lo = np.zeros(todo.size, np.int64)                              # 5
                hi = np.full(todo.size, n - 1, np.int64)
                while True:
                    act = np.flatnonzero(hi - lo > 1)
                    if act.size == 0:
                        break
                    mid = (lo[act] + hi[act]) >> 1
                    vis = ob.visible(todo[act], mid)
                    hi[act[vis]] = mid[vis]
                    lo[act[~vis]] = mid[~vis]
                res[todo] = heights[hi]
            height[s] = res
            rays += ob.rays
    height = height.reshape((observers.shape[0],) + mask.shape)
    lowest = np.fmin.reduce(height, axis=0)                                     # (+inf where no observer is reached, NaN where masked)
    cells_reached = np.isfinite(height).sum(axis=(1, 2)).astype(np.int64)
    assert height.dtype == F and lowest.dtype == F
    return height, lowest, cells_reached, rays


def linear_scan(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_norm, mask, observers, heights,
                mode=orc.MODE_BVH, scene=None):
    """visible(k) for every observer, unmasked cell and table index: bool[S][unmasked cells][n] (no range limit)."""
    scene, v, norm, observers, heights = _setup(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_norm, mask,
                                                observers, heights, scene)
    cells = np.flatnonzero((mask == 1).ravel())
    out = np.empty((observers.shape[0], cells.size, heights.size), bool)
    with np.errstate(all="ignore"):
        for s, p in enumerate(observers):
            ob = _Observer(scene, v, norm, heights, p, mode)
            for k in range(heights.size):
                out[s, :, k] = ob.visible(cells, np.full(cells.size, k, np.int64))
    return out


def index_of(height, heights):
    """The table index of every finite result (exact: results are table entries), -1 for +inf and -2 for NaN."""
    heights = np.ascontiguousarray(heights, F)
    idx = np.searchsorted(heights, np.where(np.isfinite(height), height, heights[0]))
    idx = np.minimum(idx, heights.size - 1)
    assert np.array_equal(heights[idx][np.isfinite(height)], height[np.isfinite(height)])
    return np.where(np.isfinite(height), idx, np.where(np.isnan(height), -2, -1))
