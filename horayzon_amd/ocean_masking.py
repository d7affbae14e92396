"""horayzon.ocean_masking -- from a land-sea mask and the coastline to the ``mask`` argument of ``horizon_gridded`` and
``Terrain.initialise``, on MI355X (reference: horayzon/ocean_masking.py:163-345, a SciPy k-d tree on the host).

``coastline_distance`` and ``coastline_buffer`` are here.  Contract, all in float64 with every operation
rounded once: ``d2(c, p) = ((cx - px)**2 + (cy - py)**2) + (cz - pz)**2``, ``dist_chord[c] = sqrt(min over p of d2(c, p))`` with a
correctly rounded square root (land cells NaN, no vertices: +inf) and ``mask_buffer[c] = dist_chord[c] > dist_thr`` (land cells
False).  The device index over the vertices only decides which of them are skipped, never a result.  ``coastline_buffer``
decides EVERY water cell exactly; the reference's block pre-classification (``block_size``, ``chord_max``) is validated as the
reference validates it and otherwise does not influence the result, so the two differ only where the reference's block bound is
not a bound (blocks whose cells differ much in height).

``get_gshhs_coastlines`` and ``coastline_contours`` of the reference are NOT here: they read the GSHHG shapefiles with fiona /
shapely and trace contours with scikit-image (file and network I/O).

Arrays are NumPy arrays; torch tensors on the GPU ``device`` are taken where they lie and then the result is a torch tensor on
that GPU (the convention of ``Terrain.accumulate``)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import hz_stats, ptr

last_stats = None      # hz_stats of the last call as a dict: t_bvh_s (index build), t_kernel_s (query), t_h2d_s, t_d2h_s,
                       # t_total_s, num_cells (water cells queried), scratch_bytes


def _is_tensor(a):
    return (not isinstance(a, np.ndarray)) and hasattr(a, "data_ptr")


def _prepare(arrays, dtypes, device):
    """C-contiguous arrays of the given dtypes, all NumPy or all torch tensors on cuda:device; returns (arrays, torch or None)"""
    tensors = [_is_tensor(a) for a in arrays]
    if any(tensors):
        import torch
        if not all(tensors):
            raise ValueError("torch tensors and NumPy arrays cannot be mixed")
        for a in arrays:
            if a.device.type != "cuda" or (a.device.index or 0) != device:
                raise ValueError("torch tensors must be on the GPU the call runs on (device %d)" % device)
        tdt = {np.float64: torch.float64, np.uint8: torch.uint8}
        return [a.to(tdt[dt]).contiguous() for a, dt in zip(arrays, dtypes)], torch
    return [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(arrays, dtypes)], None


def _points(pts_ecef):
    if len(pts_ecef.shape) != 2 or pts_ecef.shape[1] != 3:
        raise ValueError("'pts_ecef' must have the shape (number of vertices, 3)")


def _same_shapes(x_ecef, y_ecef, z_ecef):
    if len(x_ecef.shape) != 2 or tuple(y_ecef.shape) != tuple(x_ecef.shape) or tuple(z_ecef.shape) != tuple(x_ecef.shape):
        raise ValueError("Input data has inconsistent dimension length(s)")


def _is_bool(mask_land):
    return str(mask_land.dtype) in ("bool", "torch.bool")


def _run(sym, x_ecef, y_ecef, z_ecef, mask_land, pts_ecef, device, dist_thr=None):
    global last_stats
    _same_shapes(x_ecef, y_ecef, z_ecef)
    _points(pts_ecef)
    mask_u8 = mask_land.view(np.uint8) if isinstance(mask_land, np.ndarray) else mask_land
    (x, y, z, m, p), torch = _prepare([x_ecef, y_ecef, z_ecef, mask_u8, pts_ecef],
                                      [np.float64, np.float64, np.float64, np.uint8, np.float64], device)
    shp = tuple(x.shape)
    want_mask = dist_thr is not None
    if torch is None:
        out = np.empty(shp, np.uint8 if want_mask else np.float64)
    else:
        out = torch.empty(shp, dtype=torch.uint8 if want_mask else torch.float64, device=x.device)
    if shp[0] * shp[1] > 0:
        st = hz_stats()
        args = [ptr(x), ptr(y), ptr(z), ptr(m), shp[0], shp[1], ptr(p) if p.shape[0] else None, p.shape[0]]
        if want_mask:
            args.append(float(dist_thr))
        _lib.check(getattr(_lib.lib(), sym)(*args, ptr(out), device, C.byref(st)))
        last_stats = st.as_dict()
    if want_mask:
        return out.view(np.bool_) if torch is None else out.to(torch.bool)
    return out


def coastline_distance(x_ecef, y_ecef, z_ecef, mask_land, pts_ecef, *, device=0):
    """Minimal chord distance [metre] between every water grid cell (centre) and the coastline; arguments and checks as the
    reference (ocean_masking.py:163-212).  x_ecef, y_ecef, z_ecef: float64[y][x] ECEF coordinates [metre]; mask_land: bool[y][x];
    pts_ecef: float64[vertices][3].  Returns float64[y][x], NaN at land cells (+inf everywhere else if there is no vertex)."""
    if tuple(x_ecef.shape) != tuple(mask_land.shape):
        raise ValueError("Input data has inconsistent dimension length(s)")
    if not _is_bool(mask_land):
        raise ValueError("'mask_land' must be a boolean mask")
    return _run("hz_coastline_distance", x_ecef, y_ecef, z_ecef, mask_land, pts_ecef, device)


def _lonlat2ecef(lon, lat, ellps):
    """ECEF coordinates [metre] of points at height 0 (degrees in, float64)."""
    lon, lat = np.deg2rad(lon), np.deg2rad(lat)
    if ellps == "sphere":
        r = 6370997.0
        return r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat)
    a = 6378137.0
    f = (1.0 / 298.257222101) if ellps == "GRS80" else (1.0 / 298.257223563)
    b = a * (1.0 - f)
    e_2 = 1.0 - (b ** 2 / a ** 2)
    n = a / np.sqrt(1.0 - e_2 * np.sin(lat) ** 2)
    return n * np.cos(lat) * np.cos(lon), n * np.cos(lat) * np.sin(lon), (b ** 2 / a ** 2) * n * np.sin(lat)


def chord_max(lat, dem_res, ellps, block_size):
    """The reference's bound of the chord between a block's centre and its cells (ocean_masking.py:266-281): the diagonal of half
    a block, at height 0 on the parallel 1 degree nearer the equator than the grid's parallel of smallest absolute latitude."""
    lat = np.asarray(lat.detach().cpu() if _is_tensor(lat) else lat, dtype=np.float64)
    half = int((block_size - 1) / 2)
    lat_ini = np.maximum(np.abs(lat).min() - 1.0, 0.0)
    x, y, z = _lonlat2ecef(np.array([0.0, 0.0 + dem_res * half]), np.array([lat_ini, lat_ini + dem_res * half]), ellps)
    return np.sqrt(np.diff(x)[0] ** 2 + np.diff(y)[0] ** 2 + np.diff(z)[0] ** 2)


def coastline_buffer(x_ecef, y_ecef, z_ecef, mask_land, pts_ecef, lat, dist_thr, dem_res, ellps, block_size=(5 * 2 + 1), *,
                     device=0):
    """Mask of the grid cells whose minimal chord distance from the coastline is longer than ``dist_thr`` [metre] (True =
    outside the buffer; land cells False); arguments and checks as the reference (ocean_masking.py:217-345).  lat: float64[y]
    geographic latitude [degree]; dem_res: resolution of the DEM [degree]; ellps: "sphere", "GRS80" or "WGS84"; block_size: odd.
    ``lat``, ``dem_res``, ``ellps`` and ``block_size`` are validated and otherwise unused: every water cell is decided exactly."""
    if (tuple(x_ecef.shape) != tuple(mask_land.shape)) or (x_ecef.shape[0] != len(lat)):
        raise ValueError("Input data has inconsistent dimension length(s)")
    if not _is_bool(mask_land):
        raise ValueError("'mask_land' must be a boolean mask")
    if ellps not in ("sphere", "WGS84", "GRS80"):
        raise ValueError("invalid value for 'ellps'")
    if block_size % 2 != 1:
        raise ValueError("Integer value for 'block_size' must be uneven")
    if len(lat) and chord_max(lat, dem_res, ellps, block_size) > dist_thr:
        raise ValueError("Maximal chord distance is larger than 'dist_thr'")
    return _run("hz_coastline_buffer", x_ecef, y_ecef, z_ecef, mask_land, pts_ecef, device, dist_thr=dist_thr)
