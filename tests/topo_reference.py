"""Plain NumPy reference of the three horizon reductions -- sky view factor, visible sky fraction, positive topographic
openness (horayzon/topo_param.pyx:412-603) -- and the seeded inputs the tests feed to it and to the HIP kernels.

Two results per output, vectorised over the cells with a loop over the azimuths:

``contract``  what the reference program computes, rounding where it rounds: the azimuths' sine / cosine are the float32
              of the float64 values, the tangent of the tilted plane's own horizon is formed in float32 in the
              reference's order, ``hori_plane = float32(atan(float64(.)))``, every term is float64 and is added into a
              FLOAT32 accumulator in azimuth order (``agg = float32(float64(agg) + term)``).
``exact``     the same formulas from the same float32 inputs with every intermediate in float64 (the accumulator in
              long double): what the reductions are worth without any float32 rounding.

``|contract - exact|`` is therefore the reference's own error, and the yardstick for a kernel that evaluates its terms
otherwise.  Nothing here restates a kernel's operation sequence."""
import collections

import numpy as np

NAMES = ("svf", "vsf", "openness")
HALF_PI = np.pi / 2.0

Result = collections.namedtuple("Result", "contract exact agg_max scale")
Result.__doc__ = """contract float32 (y, x); exact float64 (y, x); agg_max float32 (y, x): the largest |accumulator| of
`contract` on the way (its float32 ulp is the grain of the sum); scale: the factor between accumulator and output."""


def topo_reference(azim, hori, vec_tilt=None, which=NAMES, perturb_ulps=0, seed=0):
    """{name: Result} for the names in `which`.  `perturb_ulps` = n moves every float64 term of `contract` by +n or -n
    float64 ulps (sign drawn from `seed`) before it is added: how much of `contract` hangs on the last bits of libm."""
    names = [which] if isinstance(which, str) else list(which)
    azim = np.asarray(azim)
    hori = np.asarray(hori)
    assert azim.dtype == np.float32 and hori.dtype == np.float32 and hori.ndim == 3 and hori.shape[2] == len(azim)
    shape, A = hori.shape[:2], len(azim)
    h = hori.reshape(-1, A)
    n = h.shape[0]
    tilted = "svf" in names or "vsf" in names
    rng = np.random.default_rng(seed)

    def nudge(term):
        if not perturb_ulps:
            return term
        sign = rng.integers(0, 2, term.shape) * 2.0 - 1.0
        return term + sign * perturb_ulps * np.spacing(np.abs(term))

    out = {}
    with np.errstate(all="ignore"):
        if tilted:
            assert vec_tilt is not None and vec_tilt.dtype == np.float32 and vec_tilt.shape == shape + (3,) and A >= 2
            t = vec_tilt.reshape(-1, 3)
            tx, ty, tz = (np.ascontiguousarray(t[:, i]) for i in range(3))
            tx64, ty64, tz64 = (v.astype(np.float64) for v in (tx, ty, tz))
            az64 = azim.astype(np.float64)
            s64, c64 = np.sin(az64), np.cos(az64)
            s32, c32 = s64.astype(np.float32), c64.astype(np.float32)          # topo_param.pyx:427-429
            spac32 = np.float32(azim[1] - azim[0])                             # :433
            scale_c = np.float64(spac32) / (2.0 * np.pi)
            scale_e = (az64[1] - az64[0]) / (2.0 * np.pi)
            agg_c = {k: np.zeros(n, np.float32) for k in ("svf", "vsf") if k in names}
            agg_m = {k: np.zeros(n, np.float32) for k in agg_c}
            agg_e = {k: np.zeros(n, np.longdouble) for k in agg_c}
            for k in range(A):
                hk = h[:, k]
                # contract (:442-458, :529-541)
                tan_c = (-s32[k] * tx) / tz - (c32[k] * ty) / tz               # float32 throughout
                plane_c = np.arctan(tan_c.astype(np.float64)).astype(np.float32)
                he = np.where(hk >= plane_c, hk, plane_c).astype(np.float64)
                if "svf" in agg_c:
                    dot = (tx * s32[k] + ty * c32[k]).astype(np.float64)        # a float32 expression in the reference
                    ce = np.cos(he)
                    term = dot * ((HALF_PI - he) - (np.sin(2.0 * he) / 2.0)) + tz64 * (ce * ce)
                    agg_c["svf"] = (agg_c["svf"].astype(np.float64) + nudge(term)).astype(np.float32)
                if "vsf" in agg_c:
                    term = 1.0 - np.cos(HALF_PI - he)
                    agg_c["vsf"] = (agg_c["vsf"].astype(np.float64) + nudge(term)).astype(np.float32)
                for name in agg_c:
                    agg_m[name] = np.fmax(agg_m[name], np.abs(agg_c[name]))
                # exact
                tan_e = -s64[k] * tx64 / tz64 - c64[k] * ty64 / tz64
                plane_e = np.arctan(tan_e)
                hk64 = hk.astype(np.float64)
                he = np.where(hk64 >= plane_e, hk64, plane_e)
                if "svf" in agg_e:
                    ce = np.cos(he)
                    agg_e["svf"] += (tx64 * s64[k] + ty64 * c64[k]) * ((HALF_PI - he) - (np.sin(2.0 * he) / 2.0)) \
                        + tz64 * (ce * ce)
                if "vsf" in agg_e:
                    agg_e["vsf"] += 1.0 - np.cos(HALF_PI - he)
            for name in agg_c:
                out[name] = Result((scale_c * agg_c[name].astype(np.float64)).astype(np.float32).reshape(shape),
                                   (scale_e * agg_e[name]).astype(np.float64).reshape(shape),
                                   agg_m[name].reshape(shape), float(scale_c))
        if "openness" in names:
            agg_c = np.zeros(n, np.float32)
            agg_m = np.zeros(n, np.float32)
            agg_e = np.zeros(n, np.longdouble)
            for k in range(A):
                hk64 = h[:, k].astype(np.float64)
                agg_c = ((agg_c.astype(np.float64) + HALF_PI) - hk64).astype(np.float32)       # :600
                agg_m = np.fmax(agg_m, np.abs(agg_c))
                agg_e += HALF_PI - hk64
            out["openness"] = Result((agg_c / np.float32(A)).reshape(shape),                   # :601
                                     (agg_e / A).astype(np.float64).reshape(shape), agg_m.reshape(shape), 1.0 / A)
    return out


def e_ref(res):
    """max |contract - exact| over the cells where both are numbers: the reference's own error on this input."""
    d = np.abs(res.contract.astype(np.float64) - res.exact)
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


# ---------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------
def make_azim(azim_num, start=0.0):
    """The azimuths of a horizon call (float32 of 2 pi i / azim_num), optionally turned by `start` radian."""
    return np.array([start + (2.0 * np.pi) / azim_num * i for i in range(azim_num)], np.float32)


def grid_shape(ncell):
    """(y, x) with y * x == ncell and more than one row where the count allows it."""
    for rows in (5, 3, 2):
        if ncell % rows == 0 and ncell > rows:
            return rows, ncell // rows
    return 1, ncell


def hori_uniform(rng, shape, azim_num, lo_deg=-30.0, hi_deg=85.0, frac_half_pi=0.0):
    """Horizons uniform in [lo, hi] degrees; `frac_half_pi` of the entries set exactly to +-float32(pi/2)."""
    hori = np.deg2rad(rng.uniform(lo_deg, hi_deg, tuple(shape) + (azim_num,))).astype(np.float32)
    if frac_half_pi > 0.0:
        pick = rng.random(hori.shape)
        hori[pick < frac_half_pi / 2.0] = np.float32(HALF_PI)
        hori[pick > 1.0 - frac_half_pi / 2.0] = -np.float32(HALF_PI)
    return hori


def tilt_up(shape):
    """Exactly (0, 0, 1) everywhere."""
    tilt = np.zeros(tuple(shape) + (3,), np.float32)
    tilt[..., 2] = 1.0
    return tilt


def tilt_slopes(rng, shape, max_slope_deg, length=(1.0, 1.0)):
    """Surface normals with slopes uniform in [0, max_slope_deg] and aspects over the full circle (the plane limits the
    horizon in every octant); `length` = (lo, hi) scales each vector by a factor drawn from that range (1, 1: unit)."""
    slope = np.deg2rad(rng.uniform(0.0, max_slope_deg, shape))
    aspect = rng.uniform(0.0, 2.0 * np.pi, shape)
    tilt = np.stack([np.sin(slope) * np.sin(aspect), np.sin(slope) * np.cos(aspect), np.cos(slope)], axis=-1)
    if length != (1.0, 1.0):
        tilt = tilt * rng.uniform(length[0], length[1], tuple(shape) + (1,))
    return np.ascontiguousarray(tilt, np.float32)


def max_slope_deg(vec_tilt):
    """Largest angle between a tilt vector and the vertical [degree] (NaN vectors ignored)."""
    t = vec_tilt.reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        ang = np.degrees(np.arccos(t[:, 2] / np.linalg.norm(t, axis=1)))
    return float(np.nanmax(ang))


def add_nans(rng, hori, frac_cells=0.02, rows=()):
    """A copy of `hori` with one NaN entry in `frac_cells` of the cells and the given rows NaN throughout."""
    hori = hori.copy()
    n0, n1, A = hori.shape
    hit = np.argwhere(rng.random((n0, n1)) < frac_cells)
    for i, j in hit:
        hori[i, j, rng.integers(A)] = np.nan
    for r in rows:
        hori[r] = np.nan
    return hori


# closed-form horizon of (cell, azimuth) for arrays too large to keep on the host: an integer hash below 2^20 mapped
# linearly to [-0.5, 1.5) radian.  Every step is exact in int64 / float32, so NumPy and a device tensor library give the same bits.
PATTERN_MUL_CELL, PATTERN_MUL_AZIM, PATTERN_BITS = 2654435761, 40503, 20


def pattern_hori(cell, k, seed, xp=np):
    """float32 horizon [radian] of int64 `cell` and `k` (broadcast against each other); `xp` is numpy or torch."""
    v = (cell * PATTERN_MUL_CELL + k * PATTERN_MUL_AZIM + seed) % (1 << PATTERN_BITS)
    v = v - (1 << (PATTERN_BITS - 2))
    if xp is np:
        return v.astype(np.float32) * np.float32(2.0 ** -(PATTERN_BITS - 1))
    return v.to(xp.float32) * (2.0 ** -(PATTERN_BITS - 1))
