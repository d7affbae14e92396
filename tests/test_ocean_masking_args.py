"""horayzon.ocean_masking (hz_coastline_distance / hz_coastline_buffer): the reference's argument checks in the reference's order,
the alias, the declarations and the exports, and the yardstick's own check.  No GPU needed: every check here fires before
anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib, ocean_masking
from tests import coast_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """Replaces the library loader: any call that reaches it fails the test (the checks must come first)."""
    calls = []

    def forbidden():
        calls.append(1)
        raise AssertionError("the library was called although the arguments are invalid")
    monkeypatch.setattr(_lib, "lib", forbidden)
    yield calls
    assert calls == []


def _args(n0=12, n1=15):
    g = cc.coast_grid(n0, n1, seed=5)
    return dict(x_ecef=g["x"], y_ecef=g["y"], z_ecef=g["z"], mask_land=g["land"], pts_ecef=g["pts"]), g


def _buffer_args(**over):
    a, g = _args()
    a.update(lat=g["lat"], dist_thr=5000.0, dem_res=g["res"], ellps="sphere")
    a.update(over)
    return a


def test_distance_checks_fire_in_the_reference_order(no_library):
    a, g = _args()
    with pytest.raises(ValueError, match="inconsistent dimension"):
        ocean_masking.coastline_distance(**dict(a, mask_land=g["land"][:, :-1]))
    with pytest.raises(ValueError, match="boolean mask"):
        ocean_masking.coastline_distance(**dict(a, mask_land=g["land"].astype(np.uint8)))
    # both wrong: the shape is reported first (ocean_masking.py:190-193)
    with pytest.raises(ValueError, match="inconsistent dimension"):
        ocean_masking.coastline_distance(**dict(a, mask_land=g["land"][:-1].astype(np.uint8)))
    # this package's own checks come after the reference's
    with pytest.raises(ValueError, match="inconsistent dimension"):
        ocean_masking.coastline_distance(**dict(a, y_ecef=g["y"][:-1]))
    with pytest.raises(ValueError, match="pts_ecef"):
        ocean_masking.coastline_distance(**dict(a, pts_ecef=g["pts"][:, :2]))


BAD_BUFFER_CALLS = [
    # (overrides, message pattern) in the order of ocean_masking.py:255-281; each case also carries every LATER defect, so the
    # message shows which check came first
    (dict(mask_land="short", ellps="mars", block_size=4, dist_thr=1.0), "inconsistent dimension"),
    (dict(lat="short", mask_land="uint8", ellps="mars", block_size=4, dist_thr=1.0), "inconsistent dimension"),
    (dict(mask_land="uint8", ellps="mars", block_size=4, dist_thr=1.0), "boolean mask"),
    (dict(ellps="mars", block_size=4, dist_thr=1.0), "invalid value for 'ellps'"),
    (dict(block_size=4, dist_thr=1.0), "must be uneven"),
    (dict(dist_thr=1.0), "Maximal chord distance is larger than 'dist_thr'"),
]


@pytest.mark.parametrize("over,pattern", BAD_BUFFER_CALLS)
def test_buffer_checks_fire_in_the_reference_order(no_library, over, pattern):
    a = _buffer_args()
    over = dict(over)
    if over.get("mask_land") == "short":
        over["mask_land"] = a["mask_land"][:, :-1]
    elif over.get("mask_land") == "uint8":
        over["mask_land"] = a["mask_land"].astype(np.uint8)
    if over.get("lat") == "short":
        over["lat"] = a["lat"][:-1]
    a.update(over)
    with pytest.raises(ValueError, match=pattern):
        ocean_masking.coastline_buffer(**a)


def test_chord_max_is_the_references_definition():
    """ocean_masking.py:266-281: the chord between (0, lat_ini) and (half * dem_res, lat_ini + half * dem_res) at height 0, with
    lat_ini one degree nearer the equator than the grid's smallest absolute latitude (not below 0)."""
    res, lat = 1.0 / 1200.0, np.array([47.5, 46.0, 45.25])
    for ellps in ("sphere", "GRS80", "WGS84"):
        for block_size, half in ((11, 5), (5, 2), (1, 0)):
            got = ocean_masking.chord_max(lat, res, ellps, block_size)
            lo, la = np.deg2rad(half * res), np.deg2rad(np.array([44.25, 44.25 + half * res]))
            if ellps == "sphere":
                n = np.array([cc.RADIUS, cc.RADIUS]); zf = 1.0
            else:
                f = 1.0 / (298.257222101 if ellps == "GRS80" else 298.257223563)
                e2 = 1.0 - (1.0 - f) ** 2
                n = 6378137.0 / np.sqrt(1.0 - e2 * np.sin(la) ** 2); zf = (1.0 - f) ** 2
            p = np.array([n * np.cos(la) * np.cos([0.0, lo]), n * np.cos(la) * np.sin([0.0, lo]), zf * n * np.sin(la)])
            want = np.sqrt(((p[:, 1] - p[:, 0]) ** 2).sum())
            assert abs(got - want) <= 1e-6 * max(want, 1e-3), (ellps, block_size)
    assert ocean_masking.chord_max(np.array([0.4, -0.2]), res, "sphere", 11) == \
        ocean_masking.chord_max(np.array([0.0]), res, "sphere", 11)
    # about 5 cells of 77 m by 93 m at 44 degrees north
    assert 550.0 < ocean_masking.chord_max(lat, res, "WGS84", 11) < 650.0


def test_signatures_match_the_reference():
    p = inspect.signature(ocean_masking.coastline_distance).parameters
    assert list(p) == ["x_ecef", "y_ecef", "z_ecef", "mask_land", "pts_ecef", "device"]      # ocean_masking.py:163
    assert p["device"].kind is inspect.Parameter.KEYWORD_ONLY and p["device"].default == 0
    p = inspect.signature(ocean_masking.coastline_buffer).parameters
    assert list(p) == ["x_ecef", "y_ecef", "z_ecef", "mask_land", "pts_ecef", "lat", "dist_thr", "dem_res", "ellps",
                       "block_size", "device"]                                            # ocean_masking.py:217-218
    assert p["block_size"].default == 11
    assert p["device"].kind is inspect.Parameter.KEYWORD_ONLY and p["device"].default == 0


def test_alias_package_has_the_module():
    import horayzon
    import horayzon.ocean_masking
    import horayzon_amd
    assert horayzon.ocean_masking is horayzon_amd.ocean_masking is ocean_masking
    assert horayzon.ocean_masking.coastline_buffer is ocean_masking.coastline_buffer
    for name in ("get_gshhs_coastlines", "coastline_contours"):      # file and network I/O: out of scope, and said so
        assert not hasattr(ocean_masking, name) and name in ocean_masking.__doc__


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    common = ["const double *x_ecef", "const double *y_ecef", "const double *z_ecef", "const uint8_t *mask_land", "int len_0",
              "int len_1", "const double *pts_ecef", "size_t num_pts"]
    want = {"hz_coastline_distance": common + ["double *dist_chord", "int device", "hz_stats *stats"],
            "hz_coastline_buffer": common + ["double dist_thr", "uint8_t *mask_buffer", "int device", "hz_stats *stats"]}
    L = _lib.lib()
    for name, params in want.items():
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S)
        assert decl, name + " is not declared"
        assert [" ".join(p.split()) for p in decl.group(1).split(",")] == params
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(params)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hz_coastline_distance" in doc and "hz_coastline_buffer" in doc


def test_c_entry_points_check_their_arguments():
    """The C entry points' own checks, before any device is touched."""
    L = _lib.lib()
    a, g = _args()
    x, y, z, p = (a[k].ctypes.data for k in ("x_ecef", "y_ecef", "z_ecef", "pts_ecef"))
    m = g["land"].view(np.uint8).ctypes.data
    out = np.zeros(g["land"].shape, np.float64)
    n0, n1 = g["land"].shape
    assert L.hz_coastline_distance(x, y, z, m, n0, n1, p, len(g["pts"]), None, 0, None) == 1
    assert b"NULL" in L.hz_last_error()
    assert L.hz_coastline_distance(x, y, z, m, n0, n1, None, 3, out.ctypes.data, 0, None) == 1
    assert L.hz_coastline_distance(x, y, z, m, 0, n1, p, len(g["pts"]), out.ctypes.data, 0, None) == 1
    assert b"dimension" in L.hz_last_error()
    assert L.hz_coastline_buffer(x, y, z, m, n0, n1, p, len(g["pts"]), 100.0, None, 0, None) == 1
    assert L.hz_coastline_buffer(x, y, z, m, n0, n1, p, 1 << 31, 100.0, out.ctypes.data, 0, None) == 1
    assert b"too many" in L.hz_last_error()


def test_fails_loudly_without_gpu():
    if _lib.device_count() > 0:
        return          # a GPU is visible: the no-device path cannot be exercised (tests/test_gpu_ocean_masking.py runs the calls)
    a, _ = _args()
    with pytest.raises(_lib.HorayzonHipError, match="no HIP device"):
        ocean_masking.coastline_distance(**a)
    with pytest.raises(_lib.HorayzonHipError, match="no HIP device"):
        ocean_masking.coastline_buffer(**_buffer_args())


def test_input_maker_gives_a_coast():
    g = cc.coast_grid(150, 200, seed=7, hurst=0.5)
    land = g["land"]
    assert land.dtype == np.bool_ and 0.2 < land.mean() < 0.8 and 1000 < len(g["pts"]) < 20000
    # every vertex lies on the sphere and half a cell from a water cell: the brute force finds it there
    assert np.allclose(np.linalg.norm(g["pts"], axis=1), cc.RADIUS, rtol=1e-12)
    d = cc.brute_distance(g["x"], g["y"], g["z"], land, g["pts"])
    assert cc.same_with_nan(d, d) and np.array_equal(np.isnan(d), land)
    cell = cc.RADIUS * np.deg2rad(g["res"])
    assert 0.3 * cell < np.nanmin(d) < 0.51 * cell


def test_yardstick_brute_force_equals_the_kd_tree_bit_for_bit():
    """What licenses SciPy's k-d tree as the yardstick of the large GPU case: on a 60 x 80 grid with a few hundred vertices its
    distances equal the brute force of the contract's d2 bit for bit."""
    spatial = pytest.importorskip("scipy.spatial")
    g = cc.coast_grid(60, 80, seed=9, hurst=0.5)
    assert 200 <= len(g["pts"]) <= 2000
    w = ~g["land"]
    q = np.stack((g["x"][w], g["y"][w], g["z"][w]), axis=1)
    kd = spatial.KDTree(g["pts"]).query(q, k=1)[0]
    assert np.array_equal(np.sqrt(cc.brute_d2min(q, g["pts"])), kd)
