"""The 16-bit horizon code (hori_dtype="uint16", quantise / dequantise, HorizonTerrain.initialise_q16, hz_*_q16): argument
checks, the declarations and the exports.  No GPU needed: every check here fires before anything reaches a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib, horizon
from horayzon_amd.shadow import HorizonTerrain, gridded_azimuths
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
DEM = (8, 9)
A = 12

NEW = ("hz_hori_quantise", "hz_hori_dequantise", "hz_horizon_gridded_q16", "hz_horizon_gridded_scene_q16",
       "hz_horizon_terrain_initialise_q16")


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


# ---- Python ------------------------------------------------------------------------------------------------------

def test_names_defaults_and_constants():
    p = inspect.signature(horizon.horizon_gridded).parameters["hori_dtype"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "float32"
    assert horizon.HORI_DTYPES == ("float32", "uint16")
    assert horizon.Q16_NAN == 0xFFFF and horizon.Q16_STEP == 1.5707963267948966 / 32767.0
    assert horizon.Q16_MAX_ERROR == horizon.Q16_STEP / 2 + 2 ** -24
    for f in (horizon.quantise, horizon.dequantise):
        p = inspect.signature(f).parameters["device"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0
    # a method of its own: initialise's arguments, then the keyword-only layout
    init = list(inspect.signature(HorizonTerrain.initialise).parameters)
    q16 = inspect.signature(HorizonTerrain.initialise_q16).parameters
    assert [n.replace("hori_q", "hori") for n in q16] == init + ["layout"]
    assert q16["layout"].kind is inspect.Parameter.KEYWORD_ONLY and q16["layout"].default == "cell_major"
    import horayzon
    assert horayzon.horizon.quantise is horizon.quantise and horayzon.horizon.dequantise is horizon.dequantise


def test_horizon_gridded_rejects_bad_hori_dtypes(no_library):
    g = cases.rough_terrain(20, 24, seed=2, offset=3)
    kw = cases.grid_kwargs(g)
    tilt = np.zeros(kw["vec_norm"].shape, np.float32)
    tilt[..., 2] = 1.0
    for bad in ("float16", "UINT16", "int16", "", None, np.uint16, 16):
        with pytest.raises(ValueError, match="unknown 'hori_dtype'"):
            horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, hori_dtype=bad)
    for layout in horizon.LAYOUTS:
        with pytest.raises(ValueError, match="no horizon to"):
            horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, hori_dtype="uint16", layout=layout,
                                    topo=("openness",), topo_only=True)
        with pytest.raises(ValueError, match="no horizon to"):
            horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, hori_dtype="uint16", layout=layout,
                                    svf_vec_tilt=tilt, svf_only=True)
    # the reference's checks and the layout's still come first
    with pytest.raises(ValueError, match="ray_algorithm"):
        horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, hori_dtype="bad", ray_algorithm="fast")
    with pytest.raises(ValueError, match="unknown 'layout'"):
        horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, hori_dtype="bad", layout="bad")


def test_horizon_gridded_reaches_the_q16_entry_point(monkeypatch):
    g = cases.rough_terrain(20, 24, seed=2, offset=3)
    kw = cases.grid_kwargs(g)
    in0, in1 = kw["vec_norm"].shape[:2]
    reached = []

    class Lib:
        def hz_horizon_gridded_q16(self, *a):
            reached.append((a[8], a[9], a[10], a[11], len(a)))     # planes, dim_in_0, dim_in_1, azim_num
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    for layout, planes in (("cell_major", 0), ("azim_major", 1)):
        hori, azim = horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, hori_dtype="uint16", layout=layout, rows=(2, 5))
        assert hori.dtype == np.uint16 and (hori == horizon.Q16_NAN).all()       # pre-filled: the stub wrote nothing
        assert hori.shape == ((8, in0, in1) if planes else (in0, in1, 8))
        assert reached[-1] == (planes, in0, in1, 8, 27)


QUANTISE_RULES = [
    (lambda: [[1.0]], TypeError, "incorrect type"),
    (lambda: np.zeros((4, 5), np.float64), ValueError, "dtype mismatch"),
    (lambda: np.zeros((4, 5), np.uint16), ValueError, "dtype mismatch"),
    (lambda: np.zeros((4, 12), np.float32)[:, ::2], ValueError, "C-contiguous"),
    (lambda: np.zeros((4, 5, 6), np.float32).T, ValueError, "C-contiguous"),
]
DEQUANTISE_RULES = [
    (lambda: [[1]], TypeError, "incorrect type"),
    (lambda: np.zeros((4, 5), np.float32), ValueError, "dtype mismatch"),
    (lambda: np.zeros((4, 5), np.int16), ValueError, "dtype mismatch"),          # (int16: tensors only)
    (lambda: np.zeros((4, 5), np.uint32), ValueError, "dtype mismatch"),
    (lambda: np.zeros((4, 12), np.uint16)[:, ::2], ValueError, "C-contiguous"),
]


@pytest.mark.parametrize("make,exc,pattern", QUANTISE_RULES)
def test_quantise_checks_its_argument(no_library, make, exc, pattern):
    with pytest.raises(exc, match=pattern):
        horizon.quantise(make())


@pytest.mark.parametrize("make,exc,pattern", DEQUANTISE_RULES)
def test_dequantise_checks_its_argument(no_library, make, exc, pattern):
    with pytest.raises(exc, match=pattern):
        horizon.dequantise(make())


def test_conversions_reject_a_host_tensor(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="not on a GPU"):
        horizon.quantise(torch.zeros((3, 4), dtype=torch.float32))
    with pytest.raises(ValueError, match="not on a GPU"):
        horizon.dequantise(torch.zeros((3, 4), dtype=torch.int16))
    with pytest.raises(ValueError, match="dtype mismatch"):
        horizon.dequantise(torch.zeros((3, 4), dtype=torch.int32))


def test_conversions_take_any_shape(monkeypatch):
    seen = []

    class Lib:
        def hz_hori_quantise(self, src, n, dst, device):
            seen.append(("q", n, device))
            return 0

        def hz_hori_dequantise(self, src, n, dst, device):
            seen.append(("d", n, device))
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    for shape in ((), (7,), (2, 3), (2, 3, 4, 5), (0, 3)):
        q = horizon.quantise(np.zeros(shape, np.float32), device=2)
        assert q.dtype == np.uint16 and q.shape == shape
        v = horizon.dequantise(np.zeros(shape, np.uint16))
        assert v.dtype == np.float32 and v.shape == shape
        n = int(np.prod(shape, dtype=np.int64))
        assert seen[-2:] == [("q", n, 2), ("d", n, 0)]


def _terrain():
    t = HorizonTerrain.__new__(HorizonTerrain)
    t._h = None
    t._shape = None
    t._hori = None
    t.device = 0
    t.last_stats = None
    return t


def _init_args(planes, **change):
    unit = np.zeros(SHAPE + (3,), np.float32)
    unit[..., 2] = 1.0
    north = np.zeros(SHAPE + (3,), np.float32)
    north[..., 1] = 1.0
    a = dict(azim=gridded_azimuths(A), hori_q=np.zeros(((A,) + SHAPE) if planes else (SHAPE + (A,)), np.uint16),
             vert_grid=np.zeros(DEM[0] * DEM[1] * 3, np.float32), dem_dim_0=DEM[0], dem_dim_1=DEM[1], offset_0=1, offset_1=1,
             vec_tilt=unit.copy(), vec_norm=unit.copy(), vec_north=north, surf_enl_fac=np.ones(SHAPE, np.float32),
             mask=np.ones(SHAPE, np.uint8), sw_dir_cor_fill=np.nan, ang_max=89.0, layout="azim_major" if planes else "cell_major")
    for k, v in change.items():
        a[k] = v(a[k]) if callable(v) else v
    return a


CELL, PLANES = SHAPE + (A,), (A,) + SHAPE
INIT_RULES = [
    # (planes, change, exception, message)
    (0, dict(hori_q=lambda a: a.tolist()), TypeError, "'hori_q' has incorrect type"),
    (0, dict(hori_q=lambda a: a.astype(np.float32)), ValueError, "dtype mismatch"),
    (1, dict(hori_q=lambda a: a.astype(np.int16)), ValueError, "dtype mismatch"),
    (0, dict(hori_q=lambda a: a[0]), ValueError, "wrong number of dimensions"),
    (1, dict(hori_q=lambda a: a[0]), ValueError, "wrong number of dimensions"),
    (0, dict(hori_q=lambda a: np.zeros(PLANES, np.uint16)), ValueError, "shape of 'hori_q'"),        # the other layout's array
    (1, dict(hori_q=lambda a: np.zeros(CELL, np.uint16)), ValueError, "shape of 'hori_q'"),
    (0, dict(hori_q=lambda a: a[:, :-1]), ValueError, "shape of 'hori_q'"),
    (1, dict(hori_q=lambda a: a[:, :-1]), ValueError, "shape of 'hori_q'"),
    (0, dict(hori_q=lambda a: a[..., :-1]), ValueError, "'azim' is not the azimuth array of horizon_gridded"),
    (1, dict(hori_q=lambda a: a[:-1]), ValueError, "'azim' is not the azimuth array of horizon_gridded"),
    (0, dict(hori_q=lambda a: np.zeros(SHAPE + (2 * A,), np.uint16)[..., ::2]), ValueError, "C-contiguous"),
    (1, dict(hori_q=lambda a: np.transpose(np.zeros(CELL, np.uint16), (2, 0, 1))), ValueError, "C-contiguous"),
    (0, dict(layout="planes"), ValueError, "unknown 'layout'"),
    (0, dict(ang_max=84.9), TypeError, "'ang_max' must be in the range"),
]


@pytest.mark.parametrize("planes,change,exc,pattern", INIT_RULES)
def test_initialise_q16_rules_fire_before_the_library(no_library, planes, change, exc, pattern):
    t = _terrain()
    with pytest.raises(exc, match=pattern):
        t.initialise_q16(**_init_args(planes, **change))
    assert t._shape is None


def test_initialise_q16_reaches_its_entry_point(monkeypatch):
    reached = []

    class Lib:
        def hz_horizon_terrain_initialise_q16(self, *a):
            reached.append((a[2], a[3], len(a)))                  # azim_num, planes
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    for planes in (0, 1):
        t = _terrain()
        t.initialise_q16(**_init_args(planes))
        assert reached[-1] == (A, planes, 19) and t._shape == SHAPE and not t.refrac_cor
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):               # a tensor that is not on the object's GPU
        _terrain().initialise_q16(**_init_args(0, hori_q=torch.zeros(CELL, dtype=torch.int16)))
    with pytest.raises(ValueError, match="dtype mismatch"):
        _terrain().initialise_q16(**_init_args(0, hori_q=torch.zeros(CELL, dtype=torch.float32)))


def test_the_float_forms_keep_rejecting_codes(no_library):
    for planes, init in ((0, HorizonTerrain.initialise), (1, HorizonTerrain.initialise_azim_major)):
        a = _init_args(planes)
        a["hori"] = a.pop("hori_q")
        del a["layout"]
        with pytest.raises(ValueError, match="dtype mismatch"):
            init(_terrain(), **a)


# ---- C ABI -------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in (
            "int hz_hori_quantise(const float *src, size_t n, uint16_t *dst, int device);",
            "int hz_hori_dequantise(const uint16_t *src, size_t n, float *dst, int device);",
            "int hz_horizon_terrain_initialise_q16(hz_horizon_terrain* t, const uint16_t* hori_q, int azim_num, int planes,"):
        assert proto in flat, proto
    # the q16 forms of the horizon call: the planes argument lists with `uint16_t *hori_q, int planes` for hori_planes
    for name in ("hz_horizon_gridded", "hz_horizon_gridded_scene"):
        pl = re.search(r"int %s_planes\((.*?)\);" % name, flat).group(1)
        q = re.search(r"int %s_q16\((.*?)\);" % name, flat).group(1)
        assert "float *hori_planes" in pl and q == pl.replace("float *hori_planes", "uint16_t *hori_q, int planes"), name
    L = _lib.lib()
    for name, n_args in zip(NEW, (4, 4, 27, 20, 19)):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args, name
    assert "horisun_coarse_route" in re.search(r"/\*[^;]*?\*/\s*int hz_horizon_terrain_initialise_q16", hdr, flags=re.S).group(0)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, name


def test_abi_revision_and_struct_sizes_are_unchanged():
    L = _lib.lib()
    assert L.hz_abi_version() == 6
    a, b = C.c_int(0), C.c_int(0)
    assert L.hz_abi_struct_sizes(C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (C.sizeof(_lib.hz_opts), C.sizeof(_lib.hz_stats)) == (96, 232)


def _err(L):
    return L.hz_last_error() or b""


def test_c_entry_points_check_their_arguments():
    """NULL pointers, odd addresses and non-positive lengths: HZ_ERR_ARG (1) and a message, before any device is touched;
    n == 0 succeeds without one."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    for f in (L.hz_hori_quantise, L.hz_hori_dequantise):
        assert f(None, 0, None, 0) == 0 and f(p, 0, p, 0) == 0
        assert f(None, 4, p, 0) == 1 and b"NULL" in _err(L)
        assert f(p, 4, None, 0) == 1 and b"NULL" in _err(L)
        assert f(p + 1, 4, p + 1, 0) == 1 and b"aligned" in _err(L)
    assert L.hz_hori_quantise(p + 2, 4, p, 0) == 1 and b"aligned" in _err(L)       # float32 at 2 mod 4
    assert L.hz_hori_dequantise(p, 4, p + 2, 0) == 1 and b"aligned" in _err(L)
    o = _lib.hz_opts()
    one_shot = lambda q, planes, d0, d1, a: L.hz_horizon_gridded_q16(      # noqa: E731
        p, 4, 4, p, p, 0, 0, q, planes, d0, d1, a, 1.0, 0.25, b"guess_constant", b"grid", p, 1, p, 1, -15.0, p, 0.0, 0.01,
        C.byref(o), None, None)
    assert one_shot(None, 0, 2, 2, 2) == 1 and b"hori_q is NULL" in _err(L)
    assert one_shot(p + 1, 0, 2, 2, 2) == 1 and b"aligned" in _err(L)
    for planes in (2, -1):
        assert one_shot(p, planes, 2, 2, 2) == 1 and b"planes must be 0 or 1" in _err(L)
    for lens in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (2, 2, -1)):
        assert one_shot(p, 1, *lens) == 1 and b"must be positive" in _err(L), lens
    o.skip_hori = 1
    for planes in (0, 1):
        assert one_shot(p, planes, 2, 2, 2) == 1 and b"nothing to lay out" in _err(L)
    assert L.hz_horizon_gridded_scene_q16(None, p, p, 0, 0, p, 0, 2, 2, 2, 1.0, 0.25, b"guess_constant", -15.0, p, 0.0, 0.01,
                                          None, None, None) == 1 and b"scene is NULL" in _err(L)
    init = lambda q, planes: L.hz_horizon_terrain_initialise_q16(          # noqa: E731
        None, q, 1, planes, None, 1, 1, 0, 0, None, None, None, 1, 1, None, None, 0.0, 89.0, None)
    assert init(p, 0) == 1 and b"terrain is NULL" in _err(L)
    assert init(p, 3) == 1 and b"planes must be 0 or 1" in _err(L)
    assert init(p + 1, 0) == 1 and b"aligned" in _err(L)


def test_q16_chunk_knob_is_accepted():
    L = _lib.lib()
    for v in (1, 100, -1):
        assert L.hz_debug_set(b"q16_chunk", v) == 0
