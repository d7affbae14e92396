"""HorizonTerrain (hz_horizon_terrain_*): argument checks, the declarations and the exports.  No GPU needed: every check
here fires before anything reaches a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import HorizonTerrain, Terrain, gridded_azimuths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
DEM = (8, 9)
A = 12


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


def _terrain(shape=SHAPE):
    """A HorizonTerrain that looks initialised to the Python checks, without a device behind it."""
    t = HorizonTerrain.__new__(HorizonTerrain)
    t._h = None
    t._shape = shape
    t._hori = None
    t.device = 0
    t.last_stats = None
    return t


def _init_args(**change):
    """Valid arguments of initialise, with `change` applied (a callable gets the valid value)."""
    unit = np.zeros(SHAPE + (3,), np.float32)
    unit[..., 2] = 1.0
    north = np.zeros(SHAPE + (3,), np.float32)
    north[..., 1] = 1.0
    a = dict(azim=gridded_azimuths(A), hori=np.zeros(SHAPE + (A,), np.float32),
             vert_grid=np.zeros(DEM[0] * DEM[1] * 3, np.float32), dem_dim_0=DEM[0], dem_dim_1=DEM[1], offset_0=1, offset_1=1,
             vec_tilt=unit.copy(), vec_norm=unit.copy(), vec_north=north, surf_enl_fac=np.ones(SHAPE, np.float32),
             mask=np.ones(SHAPE, np.uint8), sw_dir_cor_fill=np.nan, ang_max=89.0)
    for k, v in change.items():
        a[k] = v(a[k]) if callable(v) else v
    return a


def _off_unit(v):
    v = v.copy()
    v[2, 3] *= 1.01
    return v


def _shifted(azim):
    azim = azim.copy()
    azim[1] = np.nextafter(azim[1], np.float32(7.0))
    return azim


INIT_RULES = [
    # (changed arguments, exception class, message pattern): the type checks, then every rule of the table in its order
    (dict(azim=lambda a: a.tolist()), TypeError, "'azim' has incorrect type"),
    (dict(azim=lambda a: a.astype(np.float64)), ValueError, "dtype mismatch"),
    (dict(hori=lambda a: a.tolist()), TypeError, "'hori' has incorrect type"),
    (dict(hori=lambda a: a.astype(np.float64)), ValueError, "dtype mismatch"),
    (dict(hori=lambda a: a[..., 0]), ValueError, "wrong number of dimensions"),
    (dict(vec_north=lambda a: a.astype(np.float64)), ValueError, "dtype mismatch"),
    (dict(vec_north=lambda a: a[..., 0]), ValueError, "wrong number of dimensions"),
    (dict(mask=lambda a: a.astype(np.int32)), ValueError, "dtype mismatch"),
    (dict(vert_grid=lambda a: a[:-1]), ValueError, "'vert_grid', 'dem_dim_0' and 'dem_dim_1'"),
    (dict(offset_0=3), ValueError, "'offset_0', 'offset_1' and 'vec_norm'"),
    (dict(offset_1=3), ValueError, "'offset_0', 'offset_1' and 'vec_norm'"),
    (dict(vec_north=lambda a: a[:-1]), ValueError, "shape of 'vec_tilt', 'vec_norm' and/or 'vec_north'"),
    (dict(vec_norm=lambda a: a[:, :-1]), ValueError, "shape of 'vec_tilt', 'vec_norm' and/or 'vec_north'"),
    (dict(surf_enl_fac=lambda a: a[:-1]), ValueError, "shape of 'surf_enl_fac' and/or 'mask'"),
    (dict(mask=lambda a: a[:, :-1]), ValueError, "shape of 'surf_enl_fac' and/or 'mask'"),
    (dict(hori=lambda a: a[:-1]), ValueError, "shape of 'hori'"),
    (dict(hori=lambda a: a[..., :0], azim=lambda a: a[:0]), ValueError, "shape of 'hori'"),
    (dict(azim=lambda a: a[:-1]), ValueError, "'azim' is not the azimuth array of horizon_gridded"),
    (dict(azim=_shifted), ValueError, "'azim' is not the azimuth array of horizon_gridded"),
    (dict(azim=lambda a: a[::-1].copy()), ValueError, "'azim' is not the azimuth array of horizon_gridded"),
    (dict(azim=lambda a: np.linspace(0.0, 2.0 * np.pi, A, dtype=np.float32)), ValueError, "'azim' is not the azimuth array"),
    (dict(hori=lambda a: np.zeros(SHAPE + (2 * A,), np.float32)[..., ::2]), ValueError, "C-contiguous"),
    (dict(vec_north=lambda a: np.asfortranarray(a)), ValueError, "C-contiguous"),
    (dict(vec_north=_off_unit), ValueError, "'vec_tilt', 'vec_norm' and/or 'vec_north' are not normalised"),
    (dict(vec_norm=_off_unit), ValueError, "'vec_tilt', 'vec_norm' and/or 'vec_north' are not normalised"),
    (dict(vec_tilt=_off_unit), ValueError, "'vec_tilt', 'vec_norm' and/or 'vec_north' are not normalised"),
    (dict(ang_max=84.9), TypeError, "'ang_max' must be in the range"),
    (dict(ang_max=90.0), TypeError, "'ang_max' must be in the range"),
    (dict(dem_dim_0=40000, vert_grid=lambda a: np.zeros(40000 * DEM[1] * 3, np.float32)), ValueError, "32'767"),
]


@pytest.mark.parametrize("change,exc,pattern", INIT_RULES)
def test_initialise_rules_fire_before_the_library(no_library, change, exc, pattern):
    t = _terrain(shape=None)
    with pytest.raises(exc, match=pattern):
        t.initialise(**_init_args(**change))
    assert t._shape is None


def test_initialise_rules_fire_in_the_tables_order(no_library):
    """Two bad arguments: the earlier rule's message."""
    with pytest.raises(ValueError, match="shape of 'hori'"):
        _terrain(None).initialise(**_init_args(hori=lambda a: a[:-1], azim=_shifted))
    with pytest.raises(ValueError, match="azimuth array"):
        _terrain(None).initialise(**_init_args(azim=_shifted, vec_north=_off_unit))
    with pytest.raises(ValueError, match="not normalised"):
        _terrain(None).initialise(**_init_args(vec_north=_off_unit, ang_max=10.0))


def test_one_azimuth_is_legal_for_the_checks(monkeypatch):
    """azim_num = 1 passes every rule and reaches the library."""
    reached = []

    class Lib:
        def hz_horizon_terrain_initialise(self, *a):
            reached.append(a[2])
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    t = _terrain(None)
    t.initialise(**_init_args(hori=lambda a: a[..., :1].copy(), azim=lambda a: a[:1].copy()))
    assert reached == [1] and t._shape == SHAPE


def test_torch_horizon_must_be_on_the_objects_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain(None).initialise(**_init_args(hori=torch.zeros(SHAPE + (A,), dtype=torch.float32)))
    with pytest.raises(ValueError, match="dtype"):
        _terrain(None).initialise(**_init_args(hori=torch.zeros(SHAPE + (A,), dtype=torch.float64)))
    with pytest.raises(ValueError, match="dimensions"):
        _terrain(None).initialise(**_init_args(hori=torch.zeros(SHAPE, dtype=torch.float32)))


def _sun(n=5):
    return np.ones((n, 3), np.float32)


def _out(shape=SHAPE, dtype=np.float32):
    return np.zeros(shape, dtype)


BAD_ACCUMULATE = [
    (lambda: ((_sun().tolist(),), dict(sunlit_sum=_out())), TypeError, "sun_positions"),
    (lambda: ((_sun().astype(np.float64),), dict(sunlit_sum=_out())), ValueError, "dtype"),
    (lambda: ((np.ones((5, 4), np.float32),), dict(sunlit_sum=_out())), ValueError, "sun_positions"),
    (lambda: ((np.ones((0, 3), np.float32),), dict(sunlit_sum=_out())), ValueError, "sun_positions"),
    (lambda: ((_sun(), np.ones(4, np.float32)), dict(sunlit_sum=_out())), ValueError, "weights"),
    (lambda: ((_sun(), [1.0] * 5), dict(sunlit_sum=_out())), TypeError, "weights"),
    (lambda: ((_sun(),), dict()), ValueError, "at least one"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out((6, 8)))), ValueError, "incorrect shape"),
    (lambda: ((_sun(),), dict(sw_dir_cor_sum=_out(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out(SHAPE[::-1]).T)), ValueError, "C-contiguous"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out(), shadow_buffers=_out((4,) + SHAPE, np.uint8))), ValueError, "incorrect shape"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out(), sw_dir_cor_buffers=_out((5, 6, 8)))), ValueError, "incorrect shape"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out(), shadow_buffers=_out((5,) + SHAPE))), ValueError, "dtype"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_ACCUMULATE)
def test_accumulate_rules_fire_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().accumulate(*args, **kw)


def test_one_array_for_both_sums(no_library):
    out = _out()
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().accumulate(_sun(), sw_dir_cor_sum=out, sunlit_sum=out)


BAD_MAPS = [
    ("shadow", (np.ones(4, np.float32), _out(dtype=np.uint8)), ValueError, "sun_position"),
    ("shadow", (np.ones(3, np.float64), _out(dtype=np.uint8)), ValueError, "dtype"),
    ("shadow", (np.ones(3, np.float32), _out()), ValueError, "dtype"),
    ("shadow", (np.ones(3, np.float32), _out((6, 8), np.uint8)), ValueError, "incorrect shape"),
    ("sw_dir_cor", (np.ones(3, np.float32), _out(SHAPE[::-1]).T), ValueError, "C-contiguous"),
    ("sw_dir_cor", ([1.0, 1.0, 1.0], _out()), TypeError, "sun_position"),
    ("shadow_batch", (_sun(), _out((4,) + SHAPE, np.uint8)), ValueError, "sun_positions"),
    ("shadow_batch", (np.ones((0, 3), np.float32), _out((0,) + SHAPE, np.uint8)), ValueError, "sun_positions"),
    ("shadow_batch", (_sun(), _out((5, 6, 8), np.uint8)), ValueError, "incorrect shape"),
    ("sw_dir_cor_batch", (_sun(), _out((5,) + SHAPE, np.float64)), ValueError, "dtype"),
    ("sw_dir_cor_batch", (np.ones((5, 2), np.float32), _out((5,) + SHAPE)), ValueError, "sun_positions"),
    ("sw_dir_cor_batch", (_sun(), _out(SHAPE)), ValueError, "dimensions"),
]


@pytest.mark.parametrize("method,args,exc,pattern", BAD_MAPS)
def test_map_methods_check_their_arguments(no_library, method, args, exc, pattern):
    with pytest.raises(exc, match=pattern):
        getattr(_terrain(), method)(*args)


def test_not_initialised(no_library):
    t = _terrain(shape=None)
    calls = (lambda: t.shadow(np.ones(3, np.float32), _out(dtype=np.uint8)),
             lambda: t.sw_dir_cor(np.ones(3, np.float32), _out()),
             lambda: t.shadow_batch(_sun(), _out((5,) + SHAPE, np.uint8)),
             lambda: t.sw_dir_cor_batch(_sun(), _out((5,) + SHAPE)),
             lambda: t.accumulate(_sun(), sunlit_sum=_out()))
    for call in calls:
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            call()


def test_methods_have_terrains_names_and_signatures():
    for name in ("shadow", "sw_dir_cor", "shadow_batch", "sw_dir_cor_batch"):
        assert inspect.signature(getattr(HorizonTerrain, name)) == inspect.signature(getattr(Terrain, name)), name
    mine = inspect.signature(HorizonTerrain.accumulate).parameters
    theirs = inspect.signature(Terrain.accumulate).parameters
    assert list(mine)[:len(theirs)] == list(theirs)
    for name, p in theirs.items():
        assert mine[name].kind is p.kind and mine[name].default is p.default, name
    for extra in list(mine)[len(theirs):]:                        # additions are keyword only and optional
        assert mine[extra].kind is inspect.Parameter.KEYWORD_ONLY and mine[extra].default is None
    init = list(inspect.signature(HorizonTerrain.initialise).parameters)
    assert init == ["self", "azim", "hori", "vert_grid", "dem_dim_0", "dem_dim_1", "offset_0", "offset_1", "vec_tilt",
                    "vec_norm", "vec_north", "surf_enl_fac", "mask", "sw_dir_cor_fill", "ang_max"]
    assert "refrac" not in " ".join(init) and "refraction" in HorizonTerrain.__doc__


def test_alias_package_has_the_class():
    import horayzon
    assert horayzon.shadow.HorizonTerrain is HorizonTerrain


def test_gridded_azimuths_are_horizon_griddeds():
    src = inspect.getsource(__import__("horayzon_amd.horizon", fromlist=["x"]).horizon_gridded)
    assert "azim[i] = ((2 * np.pi) / azim_num * i)" in src        # the loop gridded_azimuths repeats
    for n in (1, 2, 7, 360):
        a = gridded_azimuths(n)
        assert a.dtype == np.float32 and a.shape == (n,) and a[0] == 0.0
        assert np.array_equal(a, np.array([(2 * np.pi) / n * i for i in range(n)], np.float32))


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in (
            "int hz_horizon_terrain_create(int device, hz_horizon_terrain** t);",
            "int hz_horizon_terrain_initialise(hz_horizon_terrain* t, const float* hori, int azim_num, const float* vert_grid, "
            "int dem_dim_0, int dem_dim_1, int offset_0, int offset_1, const float* vec_tilt, const float* vec_norm, "
            "const float* vec_north, int dim_in_0, int dim_in_1, const float* surf_enl_fac, const uint8_t* mask, "
            "float sw_dir_cor_fill, float ang_max, hz_stats* stats);",
            "int hz_horizon_terrain_run(hz_horizon_terrain* t, const float* sun_positions, const float* weights , int num_sun, "
            "const hz_horisun_out* out, hz_stats* stats);",
            "int hz_horizon_terrain_destroy(hz_horizon_terrain* t);"):
        assert proto in flat, proto
    L = _lib.lib()
    for name, n_args in (("hz_horizon_terrain_create", 2), ("hz_horizon_terrain_initialise", 18),
                         ("hz_horizon_terrain_run", 6), ("hz_horizon_terrain_destroy", 1)):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args
    # the struct: int32 size, then four pointers
    assert [f[0] for f in _lib.hz_horisun_out._fields_] == ["size", "shadow", "sw_dir_cor", "sw_dir_cor_sum", "sunlit_sum"]
    assert _lib.hz_horisun_out().size == C.sizeof(_lib.hz_horisun_out) == 40
    assert L.hz_abi_version() == 6                               # additive: the revision of the existing structs stays


def test_c_entry_points_check_their_arguments():
    """The C entry points' own checks, before any device is touched."""
    L = _lib.lib()
    sun = _sun()
    out = _lib.hz_horisun_out(sunlit_sum=_out().ctypes.data)
    assert L.hz_horizon_terrain_run(None, sun.ctypes.data, None, 5, C.byref(out), None) == 1
    assert b"not initialised" in L.hz_last_error()
    assert L.hz_horizon_terrain_initialise(None, None, 1, None, 1, 1, 0, 0, None, None, None, 1, 1, None, None,
                                           0.0, 89.0, None) == 1
    assert L.hz_horizon_terrain_create(0, None) == 1
    assert L.hz_horizon_terrain_destroy(None) == 0


def test_horisun_chunk_knob_is_accepted():
    L = _lib.lib()
    for v in (1, 3, 7, -1):
        assert L.hz_debug_set(b"horisun_chunk", v) == 0
    assert L.hz_debug_set(b"horisun_chunk_typo", 1) != 0
