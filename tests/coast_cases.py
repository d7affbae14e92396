"""Inputs and the yardstick of the ocean_masking tests (tests/test_ocean_masking_args.py, tests/test_gpu_ocean_masking.py).
Everything here is plain NumPy: a lon/lat grid on the sphere, a fractal land-sea mask, coastline vertices between cells of
differing mask value, and a brute force that evaluates the contract's d2 exactly as DESIGN.md section 4 writes it."""
import numpy as np

from horayzon_amd import synth

RADIUS = 6370997.0          # the reference's sphere [m]


def sphere_ecef(lon_deg, lat_deg, h=0.0):
    lon, lat = np.deg2rad(lon_deg), np.deg2rad(lat_deg)
    r = RADIUS + h
    return r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat)


def coast_grid(n0, n1, seed=7, res=1.0 / 1200.0, lat0=43.0, lon0=6.0, sea_quantile=0.55, hurst=0.8, upscale=1):
    """A grid of n0 x n1 cell centres (rows north to south) with a fractal land-sea mask: land = fractal elevation above the
    `sea_quantile` quantile, which gives islands, bays and land-locked lakes.  `upscale` > 1 makes the mask at 1 / upscale of the
    size and repeats every cell (fewer, longer coastlines; the fractal generator then stays small).  Coastline vertices: the
    midpoints (in lon / lat, at height 0) between 4-neighbours of differing mask value."""
    m0, m1 = -(-n0 // upscale), -(-n1 // upscale)
    elev = synth.fractal_elevation(m0, m1, hurst=hurst, seed=seed).astype(np.float64)
    land = elev > np.quantile(elev, sea_quantile)
    if upscale > 1:
        land = np.repeat(np.repeat(land, upscale, axis=0), upscale, axis=1)[:n0, :n1]
    land = np.ascontiguousarray(land)
    lon = lon0 + res * np.arange(n1)
    lat = lat0 - res * np.arange(n0)
    lon_2d, lat_2d = np.meshgrid(lon, lat)
    x, y, z = sphere_ecef(lon_2d, lat_2d)
    ew = land[:, 1:] != land[:, :-1]
    ns = land[1:, :] != land[:-1, :]
    p_lon = np.concatenate((0.5 * (lon_2d[:, 1:] + lon_2d[:, :-1])[ew], lon_2d[1:, :][ns]))
    p_lat = np.concatenate((lat_2d[:, 1:][ew], 0.5 * (lat_2d[1:, :] + lat_2d[:-1, :])[ns]))
    pts = np.ascontiguousarray(np.stack(sphere_ecef(p_lon, p_lat), axis=1))
    return dict(x=x, y=y, z=z, land=land, pts=pts, lon=lon, lat=lat, res=res)


def brute_d2min(q, pts, chunk=256):
    """min over p of d2(c, p) = ((cx - px) * (cx - px) + (cy - py) * (cy - py)) + (cz - pz) * (cz - pz) for the cells q f64[n][3]:
    every NumPy operation rounds once, and the minimum of identically computed values has no order."""
    out = np.full(len(q), np.inf)
    if len(pts) == 0:
        return out
    px, py, pz = pts[:, 0][None, :], pts[:, 1][None, :], pts[:, 2][None, :]
    for b in range(0, len(q), chunk):
        c = q[b:b + chunk]
        dx, dy, dz = c[:, 0:1] - px, c[:, 1:2] - py, c[:, 2:3] - pz
        out[b:b + chunk] = ((dx * dx + dy * dy) + dz * dz).min(axis=1)
    return out


def brute_distance(x, y, z, land, pts):
    """The contract's dist_chord: sqrt of the minimal d2 at water cells, NaN at land cells, +inf without vertices."""
    out = np.full(x.shape, np.nan)
    w = ~land
    out[w] = np.sqrt(brute_d2min(np.stack((x[w], y[w], z[w]), axis=1), np.asarray(pts, np.float64).reshape(-1, 3)))
    return out


def same_with_nan(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
