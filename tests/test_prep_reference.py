"""tests/prep_reference.py itself, on the CPU: pinned to the vectors the reference's own modules produced
(tests/golden/prep_reference.npz, swiss_reference.npz), and its two precisions to each other.

The golden vectors come from the reference's -ffast-math build, so apart from lonlat2ecef (float64 outputs, which the
fixture holds to 1.9e-9 m of the long-double evaluation) the bounds are the ones tests/test_gpu_prep.py uses for the
kernels; no tighter claim is made about that build.  Every figure is printed before it is asserted (pytest -s)."""
import os

import numpy as np
import pytest

from tests import prep_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_reference = pytest.mark.skipif(not R.HAVE_REFERENCE, reason=R.MISSING_PRECISION)
ELLPS = ("sphere", "GRS80", "WGS84")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "prep_reference.npz")))


def _flat(*arrays):
    return [np.ascontiguousarray(a).ravel() for a in arrays]


def _close(got, want, tol, what):
    """`got` (any precision), rounded to the fixture's type, against the fixture's array: same NaN pattern,
    max |difference| <= tol"""
    got = R.to_float64(got).reshape(want.shape).astype(want.dtype).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    m = ~np.isnan(want)
    err = float(np.abs(got[m] - want[m].astype(np.float64)).max())
    print("%-28s max |reference - fixture| = %.3g (bound %.3g)" % (what, err, tol))
    assert err <= tol, what


@needs_reference
@pytest.mark.parametrize("ellps", ELLPS)
def test_lonlat2ecef_agrees_with_the_fixture(gold, ellps):
    k = ellps + "_"
    lon, lat, h = _flat(gold[k + "lon"], gold[k + "lat"], gold[k + "h"])
    ref = R.lonlat2ecef(lon, lat, h, R.ELLPS[ellps], R.REF_TYPE)
    for got, name in zip(ref, "XYZ"):
        err = float(R.abs_err(gold[k + name].ravel(), got).max())
        print("%s %s: max |fixture - reference| = %.3g m" % (ellps, name, err))
        assert err <= 1e-8


@needs_reference
@pytest.mark.parametrize("ellps", ("GRS80", "WGS84"))
def test_lonlat2ecef_tells_the_ellipsoids_apart(gold, ellps):
    k = ellps + "_"
    other = 3 - R.ELLPS[ellps]
    lon, lat, h = _flat(gold[k + "lon"], gold[k + "lat"], gold[k + "h"])
    ref = R.lonlat2ecef(lon, lat, h, other, R.REF_TYPE)
    for got, name in zip(ref, "XYZ"):
        err = float(R.abs_err(gold[k + name].ravel(), got).max())
        print("%s fixture, other ellipsoid, %s: max |fixture - reference| = %.3g m" % (ellps, name, err))
        assert err > 1e-6


@needs_reference
@pytest.mark.parametrize("ellps", ELLPS)
def test_float64_kernels_reproduce_the_fixture(gold, ellps):
    d, k, kind = gold, ellps + "_", R.ELLPS[ellps]
    T = R.REF_TYPE
    org = d[k + "origin"]
    frame = R.make_frame(kind, org[0], org[1], T)
    for got, want in zip(frame[4:], org[2:]):
        assert float(R.abs_err(want, got)) <= 1e-8
    X, Y, Z = _flat(d[k + "X"], d[k + "Y"], d[k + "Z"])
    for got, name in zip(R.ecef2enu(X, Y, Z, kind, org[0], org[1], T), ("x_enu", "y_enu", "z_enu")):
        _close(got, d[k + name], 4e-3 * 2.0 ** -10, k + name)
    lon, lat = _flat(d[k + "lon"], d[k + "lat"])
    _close(R.surf_norm(lon, lat, T), d[k + "norm_ecef"], 1e-7, k + "norm_ecef")
    vn = d[k + "norm_ecef"].reshape(-1, 3)
    _close(R.north_dir(X, Y, Z, vn, kind, T), d[k + "north_ecef"], 1e-7, k + "north_ecef")
    _close(R.ecef2enu_vector(vn, kind, org[0], org[1], T), d[k + "norm_enu"], 1e-7, k + "norm_enu")
    _close(R.ecef2enu_vector(d[k + "north_ecef"].reshape(-1, 3), kind, org[0], org[1], T), d[k + "north_enu"], 1e-7,
           k + "north_enu")


@pytest.mark.parametrize("ellps", ELLPS)
def test_slope_evaluation_reproduces_the_fixture(gold, ellps):
    d, k = gold, ellps + "_"
    x, y, z, rot = d[k + "x_enu"], d[k + "y_enu"], d[k + "z_enu"], d[k + "rot"]
    _close(R.slope_plane_meth(x, y, z, rot), d[k + "tilt_plane"], 5e-6, k + "tilt_plane")
    _close(R.slope_plane_meth(x, y, z, rot, True), d[k + "tilt_plane_rot"], 5e-6, k + "tilt_plane_rot")
    _close(R.slope_vector_meth(x, y, z), d[k + "tilt_vector"], 2e-6, k + "tilt_vector")
    _close(R.slope_vector_meth(x, y, z, rot, True), d[k + "tilt_vector_rot"], 2e-6, k + "tilt_vector_rot")


def test_slope_evaluation_reproduces_the_planar_fixture(gold):
    d = gold
    _close(R.slope_plane_meth(d["pl_x"], d["pl_y"], d["pl_z"]), d["pl_tilt_plane"], 2e-6, "pl_tilt_plane")
    _close(R.slope_vector_meth(d["pl_x"], d["pl_y"], d["pl_z"]), d["pl_tilt_vector"], 2e-6, "pl_tilt_vector")


@needs_reference
def test_swiss_pair_reproduces_the_fixture():
    """the bounds of tests/test_gpu_prep.py::test_swiss_projection_against_reference_fixture"""
    d = np.load(os.path.join(GOLDEN, "swiss_reference.npz"))
    T = R.REF_TYPE
    e, n, h = R.wgs2swiss(*_flat(d["lon"], d["lat"], d["h_wgs"]), T)
    _close(e, d["e"], 1e-8, "e")
    _close(n, d["n"], 1e-8, "n")
    _close(h, d["h_ch"], 5e-4, "h_ch")
    lon, lat, hw = R.swiss2wgs(*_flat(d["e2"], d["n2"], d["h_ch2"]), T)
    _close(lon, d["lon2"], 1e-13, "lon2")
    _close(lat, d["lat2"], 1e-13, "lat2")
    _close(hw, d["h_wgs2"], 5e-4, "h_wgs2")


def test_float32_slope_emulation_stays_next_to_float64(gold):
    fns = {"plane": R.slope_plane_meth, "vector": R.slope_vector_meth}
    worst = 0.0
    for name, meth, x, y, z, rot, output_rot in R.slope_cases(gold):
        f64 = fns[meth](x, y, z, rot, output_rot, T=np.float64)
        f32 = fns[meth](x, y, z, rot, output_rot, T=np.float32)
        assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.shape == x.shape + (3,)
        assert np.array_equal(np.isnan(f32), np.isnan(f64)), name
        ring = np.ones(x.shape, bool)
        ring[1:-1, 1:-1] = False
        assert np.isnan(f64[ring]).all() and not np.isnan(f64[~ring]).any(), name
        if (~ring).any():
            e32 = float(np.abs(f32[~ring].astype(np.float64) - f64[~ring]).max())
            print("%-34s %-6s E32 = %.3g" % (name, meth, e32))
            worst = max(worst, e32)
            assert e32 <= 2e-7, (name, meth)
    print("worst E32 = %.3g" % worst)


def test_flat_grid_and_flip_branch():
    g = R.slope_arithmetic_grids()
    x, y, z = g["flat"]
    for fn in (R.slope_plane_meth, R.slope_vector_meth):
        for T in (np.float32, np.float64):
            t = fn(x, y, z, T=T)[1:-1, 1:-1]
            assert np.array_equal(t, np.broadcast_to(np.array([0, 0, 1], T), t.shape))
    # the raw normal of the vector method points down where y grows with the row index: the flip branch turns it up
    x, y, z = g["y_up_with_row"]
    t = R.slope_vector_meth(x, y, z)[1:-1, 1:-1]
    assert (t[..., 2] > 0.0).all()
    a_x, b_y = x[1:-1, :-2] - x[1:-1, 1:-1], y[2:, 1:-1] - y[1:-1, 1:-1]
    assert (a_x * b_y < 0.0).all()                                # (a x b).z < 0 on this grid, > 0 on the others
    x, y, z = g["rough_30m"]
    assert ((x[1:-1, :-2] - x[1:-1, 1:-1]) * (y[2:, 1:-1] - y[1:-1, 1:-1]) > 0.0).all()


def test_zero_area_patch_is_nan():
    x = np.full((3, 3), 5.0, np.float32)
    for T in (np.float32, np.float64):
        assert np.isnan(R.slope_vector_meth(x, x, x, T=T)).all()


def test_pack_vertices_length_rule():
    for n in range(41):
        length = R.vert_grid_len(n)
        assert length >= 3 * n + 16 and (length * 4) % 16 == 0 and length - (3 * n + 16) < 4
        v = np.arange(1, n + 1, dtype=np.float32)
        out = R.pack_vertices(v, v + 0.25, v + 0.5)
        assert out.dtype == np.float32 and out.shape == (length,)
        assert np.array_equal(out[:3 * n].reshape(n, 3), np.stack([v, v + 0.25, v + 0.5], 1))
        assert not out[3 * n:].any()


@pytest.mark.skipif(not (R.LONGDOUBLE_OK and R.MP is not None), reason="needs both np.longdouble and mpmath to compare them")
def test_mpmath_reference_agrees_with_longdouble():
    """the fallback reference (113-bit mpmath) and np.longdouble are the same function: they differ by long-double
    rounding only (2**-64 relative an operation, a handful of operations), far below the float64 errors the GPU tests
    measure with them.  north_dir divides a difference of ECEF-sized numbers by the length of the projected vector,
    6.4e6 m * cos(lat) >= 6.4e6 * 1.7e-3 at the 89.9 degrees these inputs reach."""
    lon, lat, h = R.geodetic_inputs(255, lat_max=89.9)
    a, b = R.lonlat2ecef(lon, lat, h, 2, np.longdouble), R.lonlat2ecef(lon, lat, h, 2, R.MP)
    for u, v in zip(a, b):
        assert R.abs_err(u, v).max() <= 6.4e6 * 2.0 ** -60
    X, Y, Z = (R.to_float64(v) for v in a)
    vn = R.surf_norm(lon, lat, np.float64).astype(np.float32)
    pairs = ((R.surf_norm(lon, lat, np.longdouble), R.surf_norm(lon, lat, R.MP), 2.0 ** -60),
             (R.north_dir(X, Y, Z, vn, 1, np.longdouble), R.north_dir(X, Y, Z, vn, 1, R.MP), 8 * 2.0 ** -64 / 1.7e-3),
             (np.stack(R.ecef2enu(X, Y, Z, 2, 8.0, 47.0, np.longdouble)), np.stack(R.ecef2enu(X, Y, Z, 2, 8.0, 47.0, R.MP)),
              6.4e6 * 2.0 ** -58),
             (R.ecef2enu_vector(vn, 0, -179.5, -60.0, np.longdouble), R.ecef2enu_vector(vn, 0, -179.5, -60.0, R.MP),
              2.0 ** -60))
    for u, v, tol in pairs:
        assert R.abs_err(u, v).max() <= tol
    lon, lat, h = R.swiss_inputs(64)
    for u, v in zip(R.wgs2swiss(lon, lat, h, np.longdouble), R.wgs2swiss(lon, lat, h, R.MP)):
        assert R.abs_err(u, v).max() <= 2.6e6 * 2.0 ** -60


def test_ulp32():
    x = np.array([1.0, 1.0 - 2.0 ** -30, 0.75, -3.0, 0.0, 1e-46, 6.1e-17])
    want = [2.0 ** -23, 2.0 ** -24, 2.0 ** -24, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149, float(np.spacing(np.float32(6.1e-17)))]
    assert np.array_equal(R.ulp32(x), want)


@needs_reference
def test_measured_bounds_see_a_wrong_kernel():
    """What tests/test_gpu_prep_reference.py would say of two subtly wrong kernels, with the float64 evaluation standing
    in for the device: the two flattening constants swapped in lonlat2ecef (0.11 mm at most), and one product of ecef2enu
    evaluated in float32.  Both leave the bounds by orders of magnitude; the honest evaluation is inside by construction."""
    lon, lat, h = R.geodetic_inputs(257)
    for kind in (1, 2):
        ref = R.lonlat2ecef(lon, lat, h, kind, R.REF_TYPE)
        good = R.lonlat2ecef(lon, lat, h, kind, np.float64)
        bad = R.lonlat2ecef(lon, lat, h, 3 - kind, np.float64)
        for r, g, b in zip(ref, good, bad):
            E = max(float(R.abs_err(g, r).max()), float(np.spacing(6.4e6)))
            print("lonlat2ecef kind %d: E = %.3g, swapped ellipsoid off by %.3g" % (kind, E, float(R.abs_err(b, r).max())))
            assert R.abs_err(b, r).max() > 100 * 4 * E
    lon, lat, h = R.patch_inputs(257, 8.0, 47.0)
    X, Y, Z = (R.to_float64(v) for v in R.lonlat2ecef(lon, lat, h, 2, np.float64))
    ref = R.ecef2enu(X, Y, Z, 2, 8.0, 47.0, R.REF_TYPE)[0]
    good = R.ecef2enu(X, Y, Z, 2, 8.0, 47.0, np.float64)[0]
    sin_lon, cos_lon, _, _, x_or, y_or, _ = R.make_frame(2, 8.0, 47.0, np.float64)
    bad = -sin_lon * (X - x_or) + (np.float32(cos_lon) * (Y - y_or).astype(np.float32)).astype(np.float64)
    E = float(R.abs_err(good, ref).max())
    bound = 0.5 * R.ulp32(ref) + 4 * E
    print("ecef2enu x: E = %.3g, float32 product off by up to %.3g beyond the bound" % (E, float((R.abs_err(bad, ref) - bound).max())))
    assert (R.abs_err(good.astype(np.float32), ref) <= bound).all()
    assert (R.abs_err(bad.astype(np.float32), ref) > bound).mean() > 0.1
