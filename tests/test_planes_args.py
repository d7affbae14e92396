"""The azimuth-major horizon layout (layout="azim_major", hz_*_planes): argument checks, the declarations and the exports.
No GPU needed: every check here fires before anything reaches a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib, horizon, topo_param
from horayzon_amd.shadow import HorizonTerrain, gridded_azimuths
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
DEM = (8, 9)
A = 12

NEW = ("hz_horizon_gridded_planes", "hz_horizon_gridded_scene_planes", "hz_hori_to_planes", "hz_hori_from_planes",
       "hz_topo_params_planes", "hz_horizon_terrain_initialise_planes")


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

def test_layout_is_keyword_only_and_defaults_to_cell_major():
    for f in (horizon.horizon_gridded, topo_param.sky_view_factor, topo_param.visible_sky_fraction,
              topo_param.topographic_openness, topo_param.topo_parameters):
        p = inspect.signature(f).parameters["layout"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "cell_major", f.__name__
    assert horizon.LAYOUTS == ("cell_major", "azim_major")
    # HorizonTerrain: a method of its own with initialise's arguments (initialise keeps its list)
    assert list(inspect.signature(HorizonTerrain.initialise_azim_major).parameters) == \
        list(inspect.signature(HorizonTerrain.initialise).parameters)
    import horayzon
    assert horayzon.horizon.to_azim_major is horizon.to_azim_major and horayzon.horizon.to_cell_major is horizon.to_cell_major


def test_horizon_gridded_rejects_bad_layouts(no_library):
    g = cases.rough_terrain(20, 24, seed=2, offset=3)
    kw = cases.grid_kwargs(g)
    tilt = np.zeros(kw["vec_norm"].shape, np.float32)
    tilt[..., 2] = 1.0
    for bad in ("planes", "AZIM_MAJOR", "", None, 1):
        with pytest.raises(ValueError, match="unknown 'layout'"):
            horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, layout=bad)
    with pytest.raises(ValueError, match="nothing|no horizon to lay out"):
        horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, layout="azim_major", topo=("openness",), topo_only=True)
    with pytest.raises(ValueError, match="nothing|no horizon to lay out"):
        horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, layout="azim_major", svf_vec_tilt=tilt, svf_only=True)
    # the reference's checks still come first
    with pytest.raises(ValueError, match="ray_algorithm"):
        horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, layout="bad", ray_algorithm="fast")


CONVERT_RULES = [
    (lambda: [[1.0]], TypeError, "incorrect type"),
    (lambda: np.zeros((4, 5), np.float32), ValueError, "wrong number of dimensions"),
    (lambda: np.zeros((4, 5, 6, 2), np.float32), ValueError, "wrong number of dimensions"),
    (lambda: np.zeros((4, 5, 6), np.float64), ValueError, "dtype mismatch"),
    (lambda: np.zeros((4, 0, 6), np.float32), ValueError, "shape"),
    (lambda: np.zeros((4, 5, 12), np.float32)[..., ::2], ValueError, "C-contiguous"),
    (lambda: np.transpose(np.zeros((4, 5, 6), np.float32), (2, 0, 1)), ValueError, "C-contiguous"),
]


@pytest.mark.parametrize("make,exc,pattern", CONVERT_RULES)
def test_conversions_check_their_argument(no_library, make, exc, pattern):
    for f in (horizon.to_azim_major, horizon.to_cell_major):
        with pytest.raises(exc, match=pattern):
            f(make())


def test_conversions_reject_a_host_tensor(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="not on a GPU"):
        horizon.to_azim_major(torch.zeros((3, 4, 5), dtype=torch.float32))


def _topo_args():
    azim = gridded_azimuths(A)
    planes = np.zeros((A,) + SHAPE, np.float32)
    tilt = np.zeros(SHAPE + (3,), np.float32)
    tilt[..., 2] = 1.0
    return azim, planes, tilt


TOPO_RULES = [
    # (layout, change of (azim, planes, tilt), message, does the openness -- no vec_tilt -- refuse it too?)
    ("columns", lambda a, p, t: (a, p, t), "unknown 'layout'", True),
    ("azim_major", lambda a, p, t: (a, p[0], t), "shapes", True),                                   # wrong rank
    ("azim_major", lambda a, p, t: (a, np.zeros(SHAPE + (A,), np.float32), t), "shapes", True),      # a cell-major array
    ("azim_major", lambda a, p, t: (a, p[:, :-1], t), "shapes", False),                             # cells disagree with vec_tilt
    ("azim_major", lambda a, p, t: (a[:-1], p, t), "shapes", True),                                 # A disagrees with azim
    ("azim_major", lambda a, p, t: (a, p.astype(np.float64), t), "data type", True),
    ("azim_major", lambda a, p, t: (a, np.zeros((A, SHAPE[0], 2 * SHAPE[1]), np.float32)[..., ::2], t), "C-contiguous", True),
]


@pytest.mark.parametrize("layout,change,pattern,openness_too", TOPO_RULES)
def test_topo_param_checks_planes(no_library, layout, change, pattern, openness_too):
    azim, planes, tilt = change(*_topo_args())
    for f in (topo_param.sky_view_factor, topo_param.visible_sky_fraction):
        with pytest.raises(ValueError, match=pattern):
            f(azim, planes, tilt, layout=layout)
    with pytest.raises(ValueError, match=pattern):
        topo_param.topo_parameters(azim, planes, tilt, layout=layout)
    if openness_too:
        with pytest.raises(ValueError, match=pattern):
            topo_param.topographic_openness(azim, planes, layout=layout)
        with pytest.raises(ValueError, match=pattern):
            topo_param.topo_parameters(azim, planes, which="openness", layout=layout)


def test_topo_param_one_azimuth_on_planes(no_library):
    azim, planes, tilt = _topo_args()
    with pytest.raises(ValueError, match="shapes"):              # azim[1] - azim[0] is read
        topo_param.sky_view_factor(azim[:1], planes[:1], tilt, layout="azim_major")


def _terrain():
    t = HorizonTerrain.__new__(HorizonTerrain)
    t._h = None
    t._shape = None
    t._hori = None
    t.device = 0
    t.last_stats = None
    return t


def _init_args(**change):
    unit = np.zeros(SHAPE + (3,), np.float32)
    unit[..., 2] = 1.0
    north = np.zeros(SHAPE + (3,), np.float32)
    north[..., 1] = 1.0
    a = dict(azim=gridded_azimuths(A), hori=np.zeros((A,) + SHAPE, np.float32),
             vert_grid=np.zeros(DEM[0] * DEM[1] * 3, np.float32), dem_dim_0=DEM[0], dem_dim_1=DEM[1], offset_0=1, offset_1=1,
             vec_tilt=unit.copy(), vec_norm=unit.copy(), vec_north=north, surf_enl_fac=np.ones(SHAPE, np.float32),
             mask=np.ones(SHAPE, np.uint8), sw_dir_cor_fill=np.nan, ang_max=89.0)
    for k, v in change.items():
        a[k] = v(a[k]) if callable(v) else v
    return a


INIT_RULES = [
    (dict(hori=lambda a: a.tolist()), TypeError, "'hori' has incorrect type"),
    (dict(hori=lambda a: a.astype(np.float64)), ValueError, "dtype mismatch"),
    (dict(hori=lambda a: a[0]), ValueError, "wrong number of dimensions"),
    (dict(hori=lambda a: np.zeros(SHAPE + (A,), np.float32)), ValueError, "shape of 'hori'"),          # a cell-major array
    (dict(hori=lambda a: a[:, :-1]), ValueError, "shape of 'hori'"),
    (dict(hori=lambda a: a[:0], azim=lambda a: a[:0]), ValueError, "shape of 'hori'"),
    (dict(azim=lambda a: a[:-1]), ValueError, "'azim' is not the azimuth array of horizon_gridded"),   # A disagrees with azim
    (dict(hori=lambda a: a[:-1]), ValueError, "'azim' is not the azimuth array of horizon_gridded"),
    (dict(hori=lambda a: np.zeros((A, SHAPE[0], 2 * SHAPE[1]), np.float32)[..., ::2]), ValueError, "C-contiguous"),
    (dict(hori=lambda a: np.transpose(np.zeros(SHAPE + (A,), np.float32), (2, 0, 1))), ValueError, "C-contiguous"),
    (dict(ang_max=84.9), TypeError, "'ang_max' must be in the range"),
]


@pytest.mark.parametrize("change,exc,pattern", INIT_RULES)
def test_initialise_azim_major_rules_fire_before_the_library(no_library, change, exc, pattern):
    t = _terrain()
    with pytest.raises(exc, match=pattern):
        t.initialise_azim_major(**_init_args(**change))
    assert t._shape is None


def test_initialise_azim_major_reaches_the_planes_entry_point(monkeypatch):
    reached = []

    class Lib:
        def hz_horizon_terrain_initialise_planes(self, *a):
            reached.append(a[2])
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    t = _terrain()
    t.initialise_azim_major(**_init_args())
    assert reached == [A] and t._shape == SHAPE
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().initialise_azim_major(**_init_args(hori=torch.zeros((A,) + SHAPE, dtype=torch.float32)))


# ---- C ABI -------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in (
            "int hz_hori_to_planes(const float *hori, int len_0, int len_1, int len_2, float *planes, int device);",
            "int hz_hori_from_planes(const float *planes, int len_0, int len_1, int len_2, float *hori, int device);",
            "int hz_topo_params_planes(const float *azim, const float *planes, const float *vec_tilt, int len_0, int len_1, "
            "int len_2, float *svf, float *vsf, float *openness, int device);",
            "int hz_horizon_terrain_initialise_planes(hz_horizon_terrain* t, const float* planes, int azim_num,"):
        assert proto in flat, proto
    # the planes forms of the horizon call: the _ex argument lists with hori_planes in place of hori_buffer
    for name in ("hz_horizon_gridded", "hz_horizon_gridded_scene"):
        ex = re.search(r"int %s_ex\((.*?)\);" % name, flat).group(1)
        pl = re.search(r"int %s_planes\((.*?)\);" % name, flat).group(1)
        assert "float *hori_buffer" in ex and pl == ex.replace("float *hori_buffer", "float *hori_planes"), name
    L = _lib.lib()
    for name, n_args in zip(NEW, (26, 19, 6, 6, 10, 18)):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, name


def test_abi_revision_and_struct_sizes_are_unchanged():
    L = _lib.lib()
    assert L.hz_abi_version() == 6
    a, b = C.c_int(0), C.c_int(0)
    assert L.hz_abi_struct_sizes(C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (C.sizeof(_lib.hz_opts), C.sizeof(_lib.hz_stats)) == (96, 232)
    assert C.sizeof(_lib.hz_topo_out) == 24 and C.sizeof(_lib.hz_horisun_out) == 40
    assert _lib.hz_stats._fields_[-1][0] == "left_redo_groups" and _lib.hz_opts._fields_[-1][0] == "left_tune"


def _err(L):
    return L.hz_last_error() or b""


def test_c_entry_points_check_their_arguments():
    """NULL pointers and non-positive lengths: HZ_ERR_ARG (1) and a message, before any device is touched."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    for f in (L.hz_hori_to_planes, L.hz_hori_from_planes):
        assert f(None, 2, 2, 2, p, 0) == 1 and b"NULL" in _err(L)
        assert f(p, 2, 2, 2, None, 0) == 1 and b"NULL" in _err(L)
        for lens in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (-1, 2, 2), (2, 2, -3)):
            assert f(p, *lens, p, 0) == 1 and b"shapes" in _err(L), lens
    f = L.hz_topo_params_planes
    assert f(None, p, p, 2, 2, 2, p, None, None, 0) == 1 and b"NULL" in _err(L)
    assert f(p, None, p, 2, 2, 2, p, None, None, 0) == 1 and b"NULL" in _err(L)
    assert f(p, p, None, 2, 2, 2, None, p, None, 0) == 1 and b"NULL" in _err(L)       # vsf needs vec_tilt
    assert f(p, p, p, 2, 2, 2, None, None, None, 0) == 1 and b"no output" in _err(L)
    for lens in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (2, -2, 2)):
        assert f(p, p, None, *lens, None, None, p, 0) == 1 and b"shapes" in _err(L), lens
    assert f(p, p, p, 2, 2, 1, p, None, None, 0) == 1 and b"shapes" in _err(L)         # svf needs two azimuths
    # the horizon calls
    o = _lib.hz_opts()
    one_shot = lambda planes, d0, d1, a: L.hz_horizon_gridded_planes(      # noqa: E731
        p, 4, 4, p, p, 0, 0, planes, d0, d1, a, 1.0, 0.25, b"guess_constant", b"grid", p, 1, p, 1, -15.0, p, 0.0, 0.01,
        C.byref(o), None, None)
    assert one_shot(None, 2, 2, 2) == 1 and b"hori_planes is NULL" in _err(L)
    for lens in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (2, 2, -1)):
        assert one_shot(p, *lens) == 1 and b"must be positive" in _err(L), lens
    o.skip_hori = 1
    assert one_shot(p, 2, 2, 2) == 1 and b"nothing to lay out" in _err(L)
    assert L.hz_horizon_gridded_scene_planes(None, p, p, 0, 0, p, 2, 2, 2, 1.0, 0.25, b"guess_constant", -15.0, p, 0.0, 0.01,
                                             None, None, None) == 1 and b"scene is NULL" in _err(L)
    # HorizonTerrain
    assert L.hz_horizon_terrain_initialise_planes(None, None, 1, None, 1, 1, 0, 0, None, None, None, 1, 1, None, None,
                                                  0.0, 89.0, None) == 1 and b"terrain is NULL" in _err(L)


def test_planes_chunk_knob_is_accepted():
    L = _lib.lib()
    for v in (1, 100, -1):
        assert L.hz_debug_set(b"planes_chunk", v) == 0
