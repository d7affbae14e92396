"""CPU reference of the distance to the horizon of a gridded horizon (clause 16).

NumPy float32 arithmetic, operation by operation as the clause states it (NumPy rounds every multiply and add on its own),
the oracle's trig tables, ``np.searchsorted`` for the table index and ``oracle.Scene.closest`` -- the minimum t over all
accepted triangles, grid mesh and outer TIN alike -- for the distances."""
import numpy as np

from oracle import oracle as orc


def table_index(elev_ang, h):
    """j = max{ i : elev_ang[i] <= h } as float64 (-1: none), NaN where h is NaN.  float32 comparisons."""
    elev_ang = np.asarray(elev_ang, np.float32)
    h = np.asarray(h, np.float32)
    j = (np.searchsorted(elev_ang, h, "right") - 1).astype(np.float64)
    j[np.isnan(h)] = np.nan                      # (searchsorted sorts NaN behind everything)
    return j


def distance_rays(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north, offset_0, offset_1, hori, dist_search,
                  hori_acc=0.25, elev_ang_low_lim=-15.0, mask=None, ray_org_elev=0.01):
    """The distance rays of the cell-major horizon ``hori`` (y, x, azim_num): ``(valid, org, dirs, tfar)`` with ``valid``
    bool (y, x, azim_num) -- mask == 1 and a horizon value that is not NaN --, ``org`` / ``dirs`` float32 (y, x, azim_num, 3)
    and ``tfar`` float32 [metre]."""
    hori = np.asarray(hori)
    assert hori.dtype == np.float32 and hori.ndim == 3
    in0, in1, azim_num = hori.shape
    assert vec_norm.shape == (in0, in1, 3)
    tb = orc.tables(azim_num, hori_acc, elev_ang_low_lim, dist_search)
    if mask is None:
        mask = np.ones((in0, in1), np.uint8)
    valid = (np.asarray(mask)[:, :, None] == 1) & ~np.isnan(hori)
    j = table_index(tb["elev_ang"], hori)
    k = np.maximum(np.where(valid, j, 0.0).astype(np.int64) - 5, 0)
    vert = np.asarray(vert_grid, np.float32)[:3 * dem_dim_0 * dem_dim_1].reshape(dem_dim_0, dem_dim_1, 3)
    vert = vert[offset_0:offset_0 + in0, offset_1:offset_1 + in1]
    norm = np.asarray(vec_norm, np.float32)
    north = np.asarray(vec_north, np.float32)
    org = vert + norm * np.float32(ray_org_elev)
    east = np.stack([north[..., 1] * norm[..., 2] - north[..., 2] * norm[..., 1],
                     north[..., 2] * norm[..., 0] - north[..., 0] * norm[..., 2],
                     north[..., 0] * norm[..., 1] - north[..., 1] * norm[..., 0]], axis=-1)
    rx = (tb["elev_cos"][k] * tb["azim_sin"][None, None, :])[..., None]
    ry = (tb["elev_cos"][k] * tb["azim_cos"][None, None, :])[..., None]
    rz = tb["elev_sin"][k][..., None]
    dirs = (east[:, :, None, :] * rx + north[:, :, None, :] * ry) + norm[:, :, None, :] * rz
    assert org.dtype == np.float32 and dirs.dtype == np.float32
    org = np.broadcast_to(org[:, :, None, :], dirs.shape)
    return valid, org, dirs, np.float32(tb["dist"])


def horizon_distance(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north, offset_0, offset_1, hori, dist_search,
                     hori_acc=0.25, elev_ang_low_lim=-15.0, mask=None, ray_org_elev=0.01, vert_simp=None, tri_ind_simp=None):
    """The reference distances, float32 (y, x, azim_num), of the cell-major float32 horizon ``hori``: NaN where the ray hits
    nothing, where the horizon value is NaN and where mask != 1."""
    valid, org, dirs, tfar = distance_rays(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north, offset_0, offset_1, hori,
                                           dist_search, hori_acc, elev_ang_low_lim, mask, ray_org_elev)
    scene = orc.Scene(vert_grid, dem_dim_0, dem_dim_1, vert_simp, tri_ind_simp)
    dist = np.full(valid.shape, np.nan, np.float32)
    if valid.any():
        hit, d = scene.closest(org[valid], dirs[valid], tfar)
        dist[valid] = np.where(hit, d, np.float32(np.nan))
    return dist


def words(a):
    """The 32-bit words of a float32 array: equality of all words is equality of all values, NaN positions included."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)
