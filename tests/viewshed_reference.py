"""CPU yardstick of Terrain.viewshed (clause 18): the classification of every (observer, cell) pair
restated in NumPy float32 -- every product, sum, square root and quotient an array operation of its own, so each is rounded
on its own -- and the one any-hit ray per pair that survives it traced by the oracle (oracle.Scene.occluded).  The GPU
tests hold the kernel to these words bit for bit."""
import numpy as np

from oracle import oracle as orc

F = np.float32

VISIBLE, FACING_AWAY, BLOCKED, MASKED, OUT_OF_RANGE = 0, 1, 2, 3, 4


def vertices(vert_grid, dem_dim_0, dem_dim_1):
    """The DEM vertices f32[dem_dim_0][dem_dim_1][3] of a packed vertex array (which may carry padding at its end)."""
    return np.ascontiguousarray(vert_grid, F)[:3 * dem_dim_0 * dem_dim_1].reshape(dem_dim_0, dem_dim_1, 3)


def viewshed(vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_tilt, vec_norm, mask, observers,
             target_elev=0.05, max_dist=None, facing=True, mode=orc.MODE_BVH, scene=None):
    """(codes u8[S][y][x], seen_count i32[y][x], cells_seen i64[S], rays) for observers f32[S][3]."""
    in0, in1 = mask.shape
    if scene is None:
        scene = orc.Scene(vert_grid, dem_dim_0, dem_dim_1)
    v = vertices(vert_grid, dem_dim_0, dem_dim_1)[offset_0:offset_0 + in0, offset_1:offset_1 + in1]
    norm = np.ascontiguousarray(vec_norm, F)
    tilt = np.ascontiguousarray(vec_tilt, F)
    observers = np.ascontiguousarray(observers, F).reshape(-1, 3)
    target = (v + norm * F(target_elev)).astype(F)                          # step 2
    assert target.dtype == F
    on = mask == 1
    codes = np.empty((observers.shape[0], in0, in1), np.uint8)
    rays = 0
    with np.errstate(all="ignore"):
        for s, p in enumerate(observers):
            d = (p[None, None, :] - target).astype(F)
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            mag = np.sqrt((dx * dx + dy * dy) + dz * dz)
            assert mag.dtype == F
            code = np.full((in0, in1), 255, np.uint8)
            code[~on] = MASKED                                              # step 1
            todo = on.copy()
            if max_dist is not None:                                        # step 3
                far = todo & (mag > F(max_dist))
                code[far] = OUT_OF_RANGE
                todo &= ~far
            here = todo & ~(mag > F(0.0))                                   # step 4
            code[here] = VISIBLE
            todo &= ~here
            u = (d / mag[..., None]).astype(F)                              # step 5
            if facing:                                                      # step 6
                dot = (tilt[..., 0] * u[..., 0] + tilt[..., 1] * u[..., 1]) + tilt[..., 2] * u[..., 2]
                assert dot.dtype == F
                away = todo & ~(dot > F(0.0))
                code[away] = FACING_AWAY
                todo &= ~away
            n = int(todo.sum())                                             # step 7
            if n:
                hit = scene.occluded(target[todo], u[todo], mag[todo], mode=mode)
                code[todo] = np.where(hit, BLOCKED, VISIBLE).astype(np.uint8)
            rays += n
            codes[s] = code
    assert (codes != 255).all()
    seen_count = (codes == VISIBLE).sum(axis=0).astype(np.int32)
    seen_count[~on] = -1
    cells_seen = (codes == VISIBLE).sum(axis=(1, 2)).astype(np.int64)
    return codes, seen_count, cells_seen, rays


def histogram(codes):
    """Cells per code 0 ... 4 of one observer's map (or of all of them)."""
    return [int((codes == c).sum()) for c in range(5)]
