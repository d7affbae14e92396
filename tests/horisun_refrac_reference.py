"""DESIGN.md section 4, clause 13 in NumPy: HorizonTerrain with atmospheric refraction.

The float32 set-up is the `refrac == 1` branch of shadow_setup (hz_shadow.hip; shadow_comp.cpp:430-446) written with explicit
np.float32 / np.float64 operations in its order; the five libm calls are the float64 NumPy function of the float32 argument
rounded to float32 -- the rounded-double yardstick oracle.crmath_sweep holds hz_crmath.h to.  The look-up is clause 10's
(tests.horisun_reference.horizon_at) fed with the bent direction, so MARGIN and CAP are that module's: the float32 part is
exact on both sides and the margin still covers the float64 chain alone."""
import numpy as np

from tests import horisun_coarse_cases as HC
from tests import horisun_reference as R

F = np.float32
D = np.float64


def _libm(fn, *x):
    """The correctly rounded float: the float64 function of the float32 arguments, rounded once."""
    with np.errstate(all="ignore"):
        return fn(*(np.asarray(a, np.float32).astype(np.float64) for a in x)).astype(np.float32)


def deg2rad_f(a):
    """shadow_comp.cpp:43-52: float in, double arithmetic, float out."""
    return ((np.asarray(a, np.float32).astype(D) / 180.0) * np.pi).astype(F)


def rad2deg_f(a):
    """shadow_comp.cpp:53-62."""
    return ((np.asarray(a, np.float32).astype(D) / np.pi) * 180.0).astype(F)


def refrac_factor(elevation):
    """k_refrac_factor (hz_shadow.hip; shadow_comp.cpp:349-354, :438-441, :156): f64 per cell,
    ((double)pressure / 101.0) * (283.0 / (273.0 + (double)temperature_degC))."""
    elevation = np.asarray(elevation, np.float32)
    temperature_ref, pressure_ref, lapse_rate = F(283.15), F(101.0), F(0.0065)
    g, r_d = F(9.81), F(287.0)
    expo = g / (r_d * lapse_rate)
    assert expo.dtype == np.float32
    with np.errstate(all="ignore"):
        temperature = temperature_ref - (lapse_rate * elevation)
        pressure = pressure_ref * _libm(np.power, temperature / temperature_ref, expo)
        temp = (temperature.astype(D) - 273.15).astype(F)                       # K2degC
        assert temperature.dtype == np.float32 and pressure.dtype == np.float32
        return (pressure.astype(D) / 101.0) * (283.0 / (273.0 + temp.astype(D)))


def atmos_refrac(elev_ang_true, fac):
    """shadow_comp.cpp:135-159 (Saemundsson) [degree]; fminf / fmaxf return the other operand for a NaN."""
    with np.errstate(all="ignore"):
        e = np.fmax(F(-1.0), np.fmin(elev_ang_true, F(90.0)))
        arg = (e.astype(D) + 10.3 / (e.astype(D) + 5.11)).astype(F)
        cor = (1.02 / _libm(np.tan, deg2rad_f(arg)).astype(D)).astype(F)
        cor = (cor.astype(D) + 0.0019279).astype(F)
        cor = (cor.astype(D) * fac).astype(F)
        return (cor.astype(D) * (1.0 / 60.0)).astype(F)


def setup_refrac(sun, vert, vec_norm, vec_tilt, fac):
    """Clause 13: s = unit(p - o) and dot_ns as in clause 10, elev_ang_true from that dot_ns, the correction, s turned about
    k = unit(s x norm) by it (Rodrigues), dot_ns from the turned s' and dot_ts = tilt . s'.  fac f64[...] = refrac_factor.
    Returns (s' f32[..., 3], dot_ns, dot_ts); a sun at the cell's zenith gives NaNs (k = 0 / 0)."""
    s, dot_ns, _ = R.setup(sun, vert, vec_norm, vec_tilt)
    sx, sy, sz = (s[..., k] for k in range(3))
    nx, ny, nz = (vec_norm[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        elev_ang_true = (90.0 - rad2deg_f(_libm(np.arccos, dot_ns)).astype(D)).astype(F)
        theta = deg2rad_f(atmos_refrac(elev_ang_true, fac))
        kx = sy * nz - sz * ny
        ky = sz * nx - sx * nz
        kz = sx * ny - sy * nx
        mag = np.sqrt((kx * kx + ky * ky) + kz * kz)
        kx, ky, kz = kx / mag, ky / mag, kz / mag
        ct, st = _libm(np.cos, theta), _libm(np.sin, theta)
        part = (((kx * sx + ky * sy) + kz * sz).astype(D) * (1.0 - ct.astype(D))).astype(F)
        rx = (sx * ct + (ky * sz - kz * sy) * st) + kx * part
        ry = (sy * ct + (kz * sx - kx * sz) * st) + ky * part
        rz = (sz * ct + (kx * sy - ky * sx) * st) + kz * part
        dot_ns = (nx * rx + ny * ry) + nz * rz
        dot_ts = (vec_tilt[..., 0] * rx + vec_tilt[..., 1] * ry) + vec_tilt[..., 2] * rz
    for a in (rx, ry, rz, dot_ns, dot_ts):
        assert a.dtype == np.float32
    return np.stack([rx, ry, rz], axis=-1), dot_ns, dot_ts


def lookup_refrac(suns, hori, vert, vec_tilt, vec_norm, vec_north, surf_enl_fac, mask, fill, ang_max, fac):
    """R.lookup for the refracted sun: code, val, margin and the `_alt` pair, the same rules applied to s'.  NaN dot products
    compare false: self-shaded (code 1, value 0) without a look-up."""
    S = suns.shape[0]
    dpm = R.dot_prod_min(ang_max)
    code = np.empty((S,) + mask.shape, np.uint8)
    val = np.empty((S,) + mask.shape, np.float32)
    code_alt, val_alt = code.copy(), val.copy()
    margin = np.full((S,) + mask.shape, np.inf)
    for i in range(S):
        s, dot_ns, dot_ts = setup_refrac(suns[i], vert, vec_norm, vec_tilt, fac)
        h, alpha, _, _, _ = R.horizon_at(s, vec_norm, vec_north, hori)
        with np.errstate(all="ignore"):
            shaded = alpha < h                          # NaN h: False
            lit_val = (dot_ts / np.maximum(dot_ns, dpm)) * surf_enl_fac
            assert lit_val.dtype == np.float32
            faces = dot_ts > F(0.0)
            inside = dot_ts > dpm
        for sh, c_out, v_out in ((shaded, code, val), (~shaded, code_alt, val_alt)):
            c_out[i] = np.where(faces, np.where(sh, 2, 0), 1)
            v_out[i] = np.where(inside & ~sh, lit_val, F(0.0))
            c_out[i][mask != 1] = 3
            v_out[i][mask != 1] = fill
        with np.errstate(all="ignore"):
            m = np.abs(alpha - h)
        margin[i] = np.where(faces & (mask == 1) & ~np.isnan(m), m, np.inf)
    return dict(code=code, val=val, margin=margin, code_alt=code_alt, val_alt=val_alt)


# ---- the cases of tests/test_gpu_horisun_refrac.py ------------------------------------------------------------------------

CHUNK_TEST = 3          # hz_debug_set("horisun_chunk", 3): S = 6 or 7 spans launches

# name: (make_case arguments, low sun, mask edit, pixel sizes of the coarse tests or None)
_SPEC = {
    "low_A360_planar": (((37, 53), (45, 61), (4, 4), 360, 6, "planar", 401), True, None, None),
    "inner_A7_random": (((37, 53), (45, 61), (4, 4), 7, 6, "random", 402), False, None, None),
    "row_A2_planar": (((1, 130), (2, 131), (1, 1), 2, 6, "planar", 403), False, None, None),
    "cell_A1_planar": (((1, 1), (1, 1), (0, 0), 1, 1, "planar", 404), False, None, None),
    "coarse_low_A360_planar": (((48, 60), (56, 68), (4, 4), 360, 7, "planar", 405), True, HC._mask_big,
                               (4, (6, 20), (48, 60), 1, (3, 5))),
    "coarse_A1_planar": (((8, 12), (8, 12), (0, 0), 1, 1, "planar", 406), False, None, ((2, 3), (8, 12), 1)),
}
NAMES = tuple(_SPEC)
COARSE = tuple(n for n in NAMES if _SPEC[n][3] is not None)
LOW_SUN = tuple(n for n in NAMES if _SPEC[n][1])
PIXELS = {n: _SPEC[n][3] for n in COARSE}

_CASES = {}


def make_case(args, low_sun, edit):
    """R.make_case plus a seeded `elevation` in [-400, 5000] m.  A low-sun case has its horizon redrawn uniformly in
    [-0.02, 0.05] rad and its suns redrawn at elevations in [-1.2, 3] degrees all round the compass at 1.5e11 m: there the
    refraction (0.3 - 0.6 degrees) decides the codes."""
    c = R.make_case(*args)
    dims, seed = args[0], args[-1]
    rng = np.random.default_rng(seed + 1000)
    c["elevation"] = rng.uniform(-400.0, 5000.0, dims).astype(np.float32)
    if low_sun:
        c["hori"] = rng.uniform(-0.02, 0.05, c["hori"].shape).astype(np.float32)
        S = c["suns"].shape[0]
        az = rng.uniform(0.0, 2.0 * np.pi, S)
        el = np.deg2rad(rng.uniform(-1.2, 3.0, S))
        d = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)
        centre = c["vert"][dims[0] // 2, dims[1] // 2].astype(np.float64)
        c["suns"] = (centre[None, :] + 1.5e11 * d).astype(np.float32)
    if edit is not None:
        edit(c["mask"])
    c["fac"] = refrac_factor(c["elevation"])
    return c


def reference(c):
    return lookup_refrac(c["suns"], c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"],
                         c["mask"], c["fill"], c["ang_max"], c["fac"])


def case(name):
    """(case, refracted reference) of a name: built once per session; the arrays are read-only afterwards."""
    if name not in _CASES:
        args, low_sun, edit, _ = _SPEC[name]
        c = make_case(args, low_sun, edit)
        ref = reference(c)
        for a in list(c.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[name] = (c, ref)
    return _CASES[name]
