"""DESIGN.md section 4, clause 14 in NumPy: HorizonTerrain.sun_times -- sunrise, sunset, sunshine duration and the number of
sunlit spells of every cell over a sun track.

The float32 set-up is clause 10's (tests.horisun_reference.setup) or, with refraction, clause 13's
(tests.horisun_refrac_reference.setup_refrac, which bends every cell's sun: no early exit); the look-up is clause 10's
(horizon_at).  The event walk below is the clause written out: float64, one NumPy operation per rounding, ascending s.
Besides the four maps `sun_times` returns what the tests need to decide which cells are held to it: per cell the smallest
|g_prev - g| over its transitions and whether any of its positions has |g| <= R.MARGIN."""
import numpy as np

from tests import horisun_reference as R
from tests import horisun_refrac_reference as RR

F = np.float32
D = np.float64
MIN_DG = 1.0e-3          # [rad] a transition between clearances closer than this is not held to the reference
CAP = 0.01               # at most this share of a case's unmasked cells may be excluded
CROSS_TOL = 1.0e-6       # |delta f| <= R.MARGIN / MIN_DG per crossing
S_TRACK = 13
CHUNK_TEST = 3           # hz_debug_set("horisun_chunk", 3): S = 13 runs in five launches, the last with one position


def sun_times(c, suns, times, fac=None):
    """Clause 14 for case `c` (the arrays of R.make_case), suns f32[S][3], times f64[S]; fac f64[y][x] = the refraction factor
    or None.  Returns dict(sunrise, sunset, duration f32[y][x], intervals i32[y][x], lit bool[S][y][x], g f64[S][y][x],
    min_dg f64[y][x] (inf: no transition), near bool[y][x])."""
    mask, fill = c["mask"], c["fill"]
    S = suns.shape[0]
    times = np.asarray(times, D)
    assert times.shape == (S,) and np.isfinite(times).all() and (np.diff(times) > 0.0).all()
    shape = mask.shape
    rise, set_, open_ = np.full(shape, np.nan), np.full(shape, np.nan), np.zeros(shape)
    dur = np.zeros(shape)
    n = np.zeros(shape, np.int32)
    g_prev, lit_prev = np.zeros(shape), np.zeros(shape, bool)
    min_dg = np.full(shape, np.inf)
    near = np.zeros(shape, bool)
    lit_all, g_all = np.empty((S,) + shape, bool), np.empty((S,) + shape)
    for s in range(S):
        if fac is None:
            s_hat, _, dot_ts = R.setup(suns[s], c["vert"], c["vec_norm"], c["vec_tilt"])
        else:
            s_hat, _, dot_ts = RR.setup_refrac(suns[s], c["vert"], c["vec_norm"], c["vec_tilt"], fac)
        h, alpha, _, _, _ = R.horizon_at(s_hat, c["vec_norm"], c["vec_north"], c["hori"])
        with np.errstate(all="ignore"):
            d = alpha - h
            beta = np.arcsin(np.fmin(np.fmax(dot_ts.astype(D), -1.0), 1.0))
            g = np.fmin(d, beta)
            lit = (dot_ts > F(0.0)) & ~(alpha < h)
        near |= np.abs(g) <= R.MARGIN
        if s == 0:
            rise = np.where(lit, times[0], rise)
            open_ = np.where(lit, times[0], open_)
            n = np.where(lit, 1, n).astype(np.int32)
        else:
            cross = lit != lit_prev
            with np.errstate(all="ignore"):
                dg = g_prev - g
                f = g_prev / dg
                f = np.where((f >= 0.0) & (f <= 1.0), f, 0.5)
                step = times[s] - times[s - 1]
                tau = times[s - 1] + f * step
            up, down = cross & lit, cross & ~lit
            min_dg = np.where(cross, np.minimum(min_dg, np.abs(dg)), min_dg)
            open_ = np.where(up, tau, open_)
            rise = np.where(up & (n == 0), tau, rise)
            n = np.where(up, n + 1, n).astype(np.int32)
            dur = np.where(down, dur + (tau - open_), dur)
            set_ = np.where(down, tau, set_)
        g_prev, lit_prev = g, lit
        lit_all[s], g_all[s] = lit, g
    dur = np.where(lit_prev, dur + (times[S - 1] - open_), dur)
    set_ = np.where(lit_prev, times[S - 1], set_)
    never = n == 0
    with np.errstate(all="ignore"):
        sunrise = np.where(never, np.nan, rise).astype(F)
        sunset = np.where(never, np.nan, set_).astype(F)
        duration = np.where(never, 0.0, dur).astype(F)
    intervals = n.copy()
    masked = mask != 1
    for a in (sunrise, sunset, duration):
        a[masked] = fill
    intervals[masked] = -1
    return dict(sunrise=sunrise, sunset=sunset, duration=duration, intervals=intervals, lit=lit_all, g=g_all, min_dg=min_dg,
                near=near)


def scored(c, ref):
    """The unmasked cells held to the reference (the exclusion rule of the issue)."""
    return (c["mask"] == 1) & ~ref["near"] & ~(ref["min_dg"] < MIN_DG)


def excluded_share(c, ref):
    unmasked = int((c["mask"] == 1).sum())
    return float(((c["mask"] == 1) & ~scored(c, ref)).sum()) / max(unmasked, 1)


def max_step(times):
    return float(np.diff(times).max()) if len(times) > 1 else 0.0


def tolerances(ref, times):
    """(event tolerance, duration tolerance) f64[y][x] for the scored cells (NaN where the reference is NaN)."""
    with np.errstate(all="ignore"):
        ev = CROSS_TOL * max_step(times)
        tol_rise = ev + np.spacing(np.abs(ref["sunrise"])).astype(D)
        tol_set = ev + np.spacing(np.abs(ref["sunset"])).astype(D)
        tol_dur = 2.0 * ref["intervals"].astype(D) * ev + np.spacing(np.abs(ref["duration"])).astype(D)
    return tol_rise, tol_set, tol_dur


# ---- the cases of tests/test_gpu_suntimes.py ------------------------------------------------------------------------------

def track(c, S=S_TRACK, el0=-10.0, el_amp=65.0):
    """A day's arc about the centre cell, as R.make_case places its suns: azimuth 60 + 240 x degrees, elevation
    el0 + el_amp sin(pi x) degrees, x = linspace(0, 1, S), at 1.5e11 m."""
    x = np.linspace(0.0, 1.0, S)
    az = np.deg2rad(60.0 + 240.0 * x)
    el = np.deg2rad(el0 + el_amp * np.sin(np.pi * x))
    n0, n1 = c["mask"].shape
    centre = c["vert"][n0 // 2, n1 // 2].astype(D)
    d = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)
    return np.ascontiguousarray((centre[None, :] + 1.5e11 * d).astype(F))


def times_uniform(S=S_TRACK):
    return 6.0 + 12.0 * np.linspace(0.0, 1.0, S)


def times_uneven(S=S_TRACK, seed=77):
    """Strictly increasing, steps between 0.25 and 2."""
    steps = np.random.default_rng(seed).uniform(0.25, 2.0, S - 1)
    return 5.5 + np.concatenate([[0.0], np.cumsum(steps)])


FLAVOURS = ("uniform", "uneven")

# name: (make_case arguments without num_sun's value changed: dims, dem, offset, A, 5, frame, seed), keyword arguments
_SPEC = {
    "inner_A360_planar": (((37, 53), (45, 61), (4, 4), 360, 5, "planar", 201), {}),       # 1961 cells: not a multiple of 256
    "inner_A7_random": (((37, 53), (45, 61), (4, 4), 7, 5, "random", 202), {}),
    "row_A2_planar": (((1, 130), (1, 130), (0, 0), 2, 5, "planar", 203), {}),
    "inner_A1_random": (((37, 53), (45, 61), (4, 4), 1, 5, "random", 204), {}),
    "cell_A360_random": (((1, 1), (3, 3), (1, 1), 360, 5, "random", 205), {}),
    "one_position": (((37, 53), (45, 61), (4, 4), 7, 5, "random", 206), {}),
    "all_masked": (((5, 9), (7, 11), (1, 1), 7, 5, "planar", 207), {}),
    "fill_minus_one": (((9, 31), (11, 33), (1, 1), 7, 5, "random", 208), dict(fill=-1.0)),
    "refrac_low_A360_planar": (((37, 53), (45, 61), (4, 4), 360, 5, "planar", 209), {}),
}
NAMES = tuple(_SPEC)
MAIN = NAMES[:5]                      # the table of the issue
MULTI_CELL = NAMES[:4]
REFRAC = "refrac_low_A360_planar"

_CASES = {}


def make(name):
    args, kw = _SPEC[name]
    if name == REFRAC:
        # horizons in [-0.02, 0.05] rad and an elevation map, as the low-sun cases of RR; the track stays below 3 degrees
        c = RR.make_case(args, True, None)
        c["suns"] = track(c, el0=-1.2, el_amp=4.2)
    else:
        c = R.make_case(*args, **kw)
        c["suns"] = track(c)
        c["fac"] = None
    if name == "one_position":
        c["suns"] = np.ascontiguousarray(c["suns"][4:5])
    if name == "all_masked":
        c["mask"][:] = 0
    S = c["suns"].shape[0]
    c["times"] = {"uniform": times_uniform(S_TRACK)[:S] if S == 1 else times_uniform(S),
                  "uneven": times_uneven(S_TRACK)[:S] if S == 1 else times_uneven(S)}
    return c


def case(name):
    """(case, {flavour: reference}) of a name: built once per session; the arrays are read-only afterwards.  The refraction
    case's references are the refracting ones; `case_plain_reference` gives the other."""
    if name not in _CASES:
        c = make(name)
        refs = {fl: sun_times(c, c["suns"], c["times"][fl], c["fac"]) for fl in FLAVOURS}
        for a in list(c.values()) + [v for r in refs.values() for v in r.values()] + list(c["times"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[name] = (c, refs)
    return _CASES[name]


_PLAIN = {}


def case_plain_reference(name, flavour):
    """The reference of a case WITHOUT refraction (for the refraction case: what the switch must change)."""
    if (name, flavour) not in _PLAIN:
        c, _ = case(name)
        _PLAIN[(name, flavour)] = sun_times(c, c["suns"], c["times"][flavour], None)
    return _PLAIN[(name, flavour)]


def runs_of_zero(codes):
    """Number of runs of code 0 along axis 0 of codes u8[S][y][x]."""
    z = codes == 0
    return (z[0].astype(np.int32) + (z[1:] & ~z[:-1]).sum(axis=0)).astype(np.int32)
