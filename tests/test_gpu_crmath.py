"""The DEVICE build of the refraction math, word for word.

hz_crmath.h (acos, tan, cos, sin, pow, hz_crm_div_const) and hz_horisun_refrac.h (deg2rad, rad2deg, atmos_refrac) are compiled
by gcc into the oracle and by hipcc into the kernels.  tests/test_oracle.py and tests/test_crmath_reference.py pin the gcc
compile (to the rounded float64 libm and to mpmath).  Here the hipcc / gfx950 compile -- whose float64 sqrt and divisions are
instruction sequences the compiler writes -- is evaluated on its own through hz_crmath_probe.hip and must give the same words:
as the mpmath fixture, and as the oracle's twin (oracle.crmath_eval / crmath_range; for deg2rad, rad2deg and atmos_refrac the
twin divides with the IEEE `/` where the device runs hz_crm_div_const, so two formulas are compared).

Every comparison is exact, on uint32 / uint64 views, NaN equal to NaN.  There is no tolerance in this file.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
D = np.float64
ACOS, TAN, COS, SIN, POW, DEG2RAD, RAD2DEG, REFRAC = range(8)
CHUNK = 1 << 24                     # elements per call of a sweep: 64 MB of float32, the largest buffer either side holds
SIGN = 0x80000000
DIRT = 0xdeadbeef


def bits(v):
    return int(np.array(v, F).view(np.uint32))


def pow_exponent():
    return F(9.81) / (F(287.0) * F(0.0065))


def differing(a, b):
    """Mask of the elements whose words differ; a NaN equals a NaN."""
    w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    assert a.dtype == b.dtype and a.shape == b.shape
    d = a.view(w) != b.view(w)
    if d.any():
        d &= ~(np.isnan(a) & np.isnan(b))
    return d


def dev_eval(hip, which, x, y=None):
    from horayzon_amd import _lib
    x = np.ascontiguousarray(x, F)
    y = None if y is None else np.ascontiguousarray(y, F)
    out = np.empty(x.shape, F)
    _lib.check(_lib.lib().hz_debug_crmath_eval(which, x.ctypes.data, None if y is None else y.ctypes.data, out.ctypes.data,
                                               x.size, 0))
    return out


def dev_range(hip, which, first_bits, stride, n, y=0.0):
    from horayzon_amd import _lib
    out = np.empty(n, F)
    _lib.check(_lib.lib().hz_debug_crmath_range(which, first_bits, stride, n, float(y), out.ctypes.data, 0))
    return out


def dev_refrac_factor(hip, elevation):
    from horayzon_amd import _lib
    out = np.empty(elevation.shape, D)
    _lib.check(_lib.lib().hz_debug_refrac_factor(elevation.ctypes.data, elevation.size, out.ctypes.data, 0))
    return out


def sweep(hip, orc, which, lo_bits, hi_bits, stride=1, y=0.0):
    """Device against host twin over the floats with the bit patterns lo_bits, lo_bits + stride, ... <= hi_bits, in chunks of
    CHUNK elements.  Returns (elements, differing elements, the first few of them as text)."""
    n = (hi_bits - lo_bits) // stride + 1
    bad, shown = 0, []
    for off in range(0, n, CHUNK):
        m = min(CHUNK, n - off)
        first = lo_bits + off * stride
        dev = dev_range(hip, which, first, stride, m, y)
        host = orc.crmath_range(which, first, stride, m, y)
        d = differing(dev, host)
        bad += int(d.sum())
        for i in np.flatnonzero(d)[:max(0, 5 - len(shown))]:
            x = np.array(first + int(i) * stride, np.uint32).view(F)
            shown.append("%s(%r [0x%08x]): device %r, host %r" % (orc.CRMATH_FUNCS[which], x, first + int(i) * stride,
                                                                   dev[i], host[i]))
    return n, bad, shown


def run_sweeps(hip, orc, plan):
    total = 0
    for which, lo, hi, stride, y in plan:
        n, bad, shown = sweep(hip, orc, which, lo, hi, stride, y)
        total += n
        print("%-12s 0x%08x .. 0x%08x stride %4d y %-10r: %9d elements, %d differ" % (orc.CRMATH_FUNCS[which], lo, hi, stride,
                                                                                  y, n, bad))
        assert bad == 0, shown
    return total


# (which, first bit pattern, last bit pattern, stride, y) -- exhaustive ranges have stride 1
ACOS_EXHAUSTIVE = [(ACOS, bits(0.5), bits(1.0), 1, 0.0), (ACOS, SIGN | bits(0.5), SIGN | bits(1.0), 1, 0.0),
                   (ACOS, bits(0.30), bits(0.52), 1, 0.0), (ACOS, SIGN | bits(0.30), SIGN | bits(0.52), 1, 0.0)]
TAN_EXHAUSTIVE = [(TAN, bits(0.02), bits(1.62), 1, 0.0)]
POW_EXHAUSTIVE = [(POW, bits(0.6), bits(1.1), 1, float(pow_exponent()))]
ACOS_SMALL = [(ACOS, bits(1e-20), bits(1e-3), 29, 0.0), (ACOS, SIGN | bits(1e-20), SIGN | bits(1e-3), 31, 0.0)]
SIN_COS = [(w, lo, hi, s, 0.0) for w in (SIN, COS)
           for lo, hi, s in ((bits(1e-12), bits(0.02), 17), (bits(0.02), bits(np.pi / 4), 3))]
FINITE = 0x7f7fffff
DEG_RAD = [(w, lo, lo + FINITE, s, 0.0) for w, s in ((DEG2RAD, 255), (RAD2DEG, 257)) for lo in (0, SIGN)]
# elevation angle [degree] over [-2, 91]: dense over the magnitudes [2^-10, 91] and [-2, -2^-10], thin below 2^-10 (where the
# formula's argument no longer moves), once per factor with strides of its own
REFRAC_SWEEP = [(REFRAC, lo, hi, s + 2 * k, y) for k, y in enumerate((0.3, 1.0, 1.06))
                for lo, hi, s in ((bits(2.0 ** -10), bits(91.0), 45), (SIGN | bits(2.0 ** -10), SIGN | bits(2.0), 45),
                                  (0, bits(2.0 ** -10), 4001), (SIGN, SIGN | bits(2.0 ** -10), 4001))]


@pytest.fixture(scope="module")
def fixture():
    d = np.load(os.path.join(ROOT, "tests", "golden", "crmath_reference.npz"))
    return {k: d[k] for k in d.files}


def test_device_words_equal_the_mpmath_fixture(hip, orc, fixture):
    """Functions 0-4 at the fixture's arguments: the device's words are mpmath's correctly rounded floats (entries flagged
    is_hard, at most 2, are held to the host build only) and the host twin's."""
    which, x, ref, hard = (fixture[k] for k in ("which", "x", "ref", "is_hard"))
    y = np.full(x.shape, fixture["pow_y"], F)
    assert fixture["pow_y"] == pow_exponent() and hard.sum() <= 2
    orc.set_libm(False)
    for k in range(5):
        m = which == k
        dev = dev_eval(hip, k, x[m], y[m])
        host = orc.crmath_eval(k, x[m], y[m])
        d_ref = differing(dev, ref[m]) & ~hard[m]
        d_host = differing(dev, host)
        print("%-5s %5d arguments: %d differ from mpmath, %d from the host build" % (orc.CRMATH_FUNCS[k], m.sum(), d_ref.sum(),
                                                                                   d_host.sum()))
        assert not d_ref.any(), [(a, b, c) for a, b, c in zip(x[m][d_ref][:5], dev[d_ref][:5], ref[m][d_ref][:5])]
        assert not d_host.any(), [(a, b, c) for a, b, c in zip(x[m][d_host][:5], dev[d_host][:5], host[d_host][:5])]


def test_device_words_equal_the_host_twin_at_the_fixture_arguments(hip, orc, fixture):
    """deg2rad, rad2deg (hz_crm_div_const on the device, `/` on the host) and atmos_refrac at all the fixture's arguments -- as
    they are (radians, cosines) and, for the angle-valued two, scaled to degrees."""
    x = fixture["x"]
    orc.set_libm(False)
    for which, arg, y in ((DEG2RAD, x, None), (DEG2RAD, x * F(57.0), None), (RAD2DEG, x, None),
                          (REFRAC, x, np.full(x.shape, 1.0, F)), (REFRAC, x * F(57.0), np.full(x.shape, 1.06, F)),
                          (REFRAC, x * F(57.0), np.full(x.shape, 0.3, F))):
        d = differing(dev_eval(hip, which, arg, y), orc.crmath_eval(which, arg, y))
        assert not d.any(), (orc.CRMATH_FUNCS[which], arg[d][:5])


def test_acos_exhaustive(hip, orc):
    """Every float of [0.5, 1], [-1, -0.5] (the float64 sqrt branches) and +-[0.30, 0.52] (the switch at 0.5 from both sides).
    30 870 080 elements; host half 0.08 s measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, ACOS_EXHAUSTIVE) > 3.0e7


def test_tan_exhaustive(hip, orc):
    """Every float of [0.02, 1.62]: the 2^-5 switch of sin_k / cos_k, the fold at pi/4, the pole at pi/2 and one float64
    division each.  53 183 776 elements; host half 0.09 s measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, TAN_EXHAUSTIVE) > 5.0e7


def test_pow_exhaustive(hip, orc):
    """Every float base of [0.6, 1.1] with the pressure formula's exponent: log's division, exp's scaling.  7 549 748
    elements; host half 0.09 s measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, POW_EXHAUSTIVE) > 7.0e6


def test_acos_small_arguments(hip, orc):
    """+-[1e-20, 1e-3] with strides 29 and 31.  31 659 257 elements; host half 0.06 s measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, ACOS_SMALL) > 3.0e7


def test_sin_cos_strided(hip, orc):
    """sin and cos over [1e-12, 0.02] (stride 17) and [0.02, pi/4] (stride 3): 63 320 836 elements in all; host half
    0.09 s measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, SIN_COS) > 6.0e7


def test_deg2rad_rad2deg_strided(hip, orc):
    """All finite floats of both signs with strides 255 / 257, subnormals included: the device's four-instruction division by
    a constant against the host's IEEE division, through the conversion to float.  33 423 872 elements; host half 0.02 s
    measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, DEG_RAD) > 3.0e7


def test_atmos_refrac_strided(hip, orc):
    """Elevation angles over [-2, 91] degrees (the clamp at -1 and 90 included) for the factors 0.3, 1.0 and 1.06.  16 171 713
    elements; host half 0.08 s measured on 8 CPUs."""
    orc.set_libm(False)
    assert run_sweeps(hip, orc, REFRAC_SWEEP) > 1.5e7


def test_specials(hip, orc):
    """The arguments outside the accurate ranges that the path can still produce: device equal to host."""
    orc.set_libm(False)
    nan, inf = F(np.nan), F(np.inf)
    one_up = np.array([bits(1.0) + 1, bits(1.0) + 2], np.uint32).view(F)
    sub = np.array([1, 0x007fffff], np.uint32).view(F)                      # smallest and largest subnormal
    yy = pow_exponent()
    cases = [(ACOS, [1.0, one_up[0], one_up[1], -1.0, nan, inf, -inf], None),
             (TAN, [0.0, -0.0, -0.3, -1.2, nan], None),
             (DEG2RAD, [-0.0, 0.0], None),
             (RAD2DEG, [-0.0, 0.0], None),
             # base 0, -0, negative, +inf, NaN, subnormal; exponent 0; |y log x| = 700 crossed on both sides (log 2 = 0.6931:
             # 1009.5 below, 1010.5 above)
             (POW, [0.0, -0.0, -0.5, inf, nan, sub[0], sub[1], 0.0, -0.0, -0.5, inf, nan, sub[0], 2.0, 0.9, 2.0, 2.0, 2.0, 2.0,
                    0.5, 0.5, 0.0, inf, 0.9],
              [yy, yy, yy, yy, yy, yy, yy, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1009.5, 1010.5, -1009.5, -1010.5, 1009.5,
               1010.5, -yy, -yy, nan])]
    for which, x, y in cases:
        x = np.array(x, F)
        y = None if y is None else np.array(y, F)
        dev, host = dev_eval(hip, which, x, y), orc.crmath_eval(which, x, y)
        print(orc.CRMATH_FUNCS[which], x, y, dev)
        d = differing(dev, host)
        assert not d.any(), (orc.CRMATH_FUNCS[which], x[d], dev[d], host[d])
    # the sign case hz_crm_div_const's comment names
    assert np.signbit(dev_eval(hip, DEG2RAD, np.array([-0.0], F)))[0]
    # +-inf: q = inf, r = fma(-c, inf, inf) = NaN on the device (documented in hz_crmath.h); the host's IEEE quotient is +-inf.
    # Exactly that difference, for both helpers, and nothing else:
    x = np.array([inf, -inf], F)
    for which in (DEG2RAD, RAD2DEG):
        dev, host = dev_eval(hip, which, x), orc.crmath_eval(which, x)
        assert np.isnan(dev).all() and np.array_equal(host, x)


def refrac_factor_restated(orc, elevation):
    """k_refrac_factor (hz_shadow.hip) in NumPy: the float32 steps in the source's order, the host twin's pow, then the
    float64 expression."""
    tref, pref, lapse = F(283.15), F(101.0), F(0.0065)
    with np.errstate(all="ignore"):
        temperature = tref - (lapse * elevation)
        ratio = temperature / tref
        pressure = pref * orc.crmath_eval(POW, ratio, np.full(ratio.shape, pow_exponent(), F))
        temp = (temperature.astype(D) - 273.15).astype(F)
        assert temperature.dtype == F and pressure.dtype == F
        return (pressure.astype(D) / 101.0) * (283.0 / (273.0 + temp.astype(D)))


def test_refraction_factor(hip, orc):
    """hz_debug_refrac_factor = the kernel Terrain and HorizonTerrain.refraction run, against its restatement, on float64
    words.  Elevations: the floats around 283.15 / 0.0065 m (the temperature crosses zero: pow of +0 and of a negative base),
    one far above it (NaN), NaN, +-inf, then -500 ... 9000 m at random.  Lengths 1 (a lone thread), 63 / 64 / 65 (a wave), 257
    (a second block) and 2^20 + 3."""
    orc.set_libm(False)
    rng = np.random.default_rng(7)
    zero_t = (bits(283.15 / 0.0065) + np.arange(-8, 9)).astype(np.uint32).view(F)
    elevation = np.concatenate([np.array([1234.5], F), zero_t, np.array([1.0e5, np.nan, np.inf, -np.inf], F),
                                rng.uniform(-500.0, 9000.0, (1 << 20) + 3 - 22).astype(F)])
    assert elevation.size == (1 << 20) + 3
    want = refrac_factor_restated(orc, elevation)
    assert np.isnan(want[18:22]).all() and np.isfinite(want[22:]).all() and (want[22:] > 0.25).all() and (want[22:] < 1.1).all()
    assert (want[1:18] == 0).any()                       # the temperature ratio reaches 0 among the floats around the crossing
    for n in (1, 63, 64, 65, 257, (1 << 20) + 3):
        got = dev_refrac_factor(hip, elevation[:n].copy())
        d = differing(got, want[:n])
        assert not d.any(), (n, elevation[:n][d][:5], got[d][:5], want[:n][d][:5])


def test_the_comparison_sees_one_ulp(hip, orc):
    """Not vacuous: with the oracle on the platform's acosf / tanf (not correctly rounded: tests/test_oracle.py measures
    0.2 % / 2 % of the arguments off by one ulp on glibc 2.35) the same exhaustive comparisons must find differing words."""
    counts = {}
    orc.set_libm(True)
    try:
        for name, plan in (("acos", ACOS_EXHAUSTIVE[:1]), ("tan", TAN_EXHAUSTIVE)):
            (which, lo, hi, stride, y), = plan
            n, bad, _ = sweep(hip, orc, which, lo, hi, stride, y)
            counts[name] = (n, bad)
    finally:
        orc.set_libm(False)
    for name, (n, bad) in counts.items():
        print("%s: %d of %d words differ from the platform libm (%.3f %%)" % (name, bad, n, 100.0 * bad / n))
    assert counts["acos"][1] > 0 and counts["tan"][1] > 0


def test_hook_lengths_and_untouched_surplus(hip, orc):
    """n = 0: no launch, output untouched.  n = 1, 255, 256, 257 (one thread, a block less one, a block, a block and one)
    into a longer dirty buffer: n correct words, the surplus untouched -- for the three hooks."""
    from horayzon_amd import _lib
    L = _lib.lib()
    orc.set_libm(False)
    rng = np.random.default_rng(11)
    for n in (0, 1, 255, 256, 257):
        x = rng.uniform(-1.0, 1.0, n + 64).astype(F)
        y = np.full(n + 64, pow_exponent(), F)
        for which in (ACOS, POW, REFRAC):
            out = np.full(n + 64, DIRT, np.uint32)
            _lib.check(L.hz_debug_crmath_eval(which, x.ctypes.data, y.ctypes.data, out.ctypes.data, n, 0))
            assert (out[n:] == DIRT).all()
            assert not differing(out[:n].view(F), orc.crmath_eval(which, x[:n], y[:n])).any()
            out = np.full(n + 64, DIRT, np.uint32)
            _lib.check(L.hz_debug_crmath_range(which, bits(0.7) - 100, 3, n, float(y[0]), out.ctypes.data, 0))
            assert (out[n:] == DIRT).all()
            assert not differing(out[:n].view(F), orc.crmath_range(which, bits(0.7) - 100, 3, n, float(y[0]))).any()
        # y = NULL for a one-argument function
        out = np.full(n + 64, DIRT, np.uint32)
        _lib.check(L.hz_debug_crmath_eval(TAN, x.ctypes.data, None, out.ctypes.data, n, 0))
        assert (out[n:] == DIRT).all() and not differing(out[:n].view(F), orc.crmath_eval(TAN, x[:n])).any()
        elevation = rng.uniform(-500.0, 9000.0, n + 64).astype(F)
        out64 = np.full(n + 64, DIRT, np.uint64)
        _lib.check(L.hz_debug_refrac_factor(elevation.ctypes.data, n, out64.ctypes.data, 0))
        assert (out64[n:] == DIRT).all()
        assert not differing(out64[:n].view(D), refrac_factor_restated(orc, elevation[:n])).any()
    # a function index outside 0 ... 7 is refused
    out = np.zeros(4, F)
    assert L.hz_debug_crmath_range(8, 0, 1, 4, C.c_float(0.0), out.ctypes.data, 0) != 0
    assert L.hz_debug_crmath_range(-1, 0, 1, 4, C.c_float(0.0), out.ctypes.data, 0) != 0
