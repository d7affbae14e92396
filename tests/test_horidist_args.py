"""The horizon distance (horizon.horizon_distance, horizon_gridded(hori_dist=True), hz_horizon_distance*, hz_horizon_gridded*_dist):
signatures, argument checks, the declarations and the exports.  No GPU needed: every check here fires before anything
reaches a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib, horizon
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hz_horizon_distance", "hz_horizon_distance_scene", "hz_horizon_gridded_dist", "hz_horizon_gridded_scene_dist")
A = 8


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


def _grid():
    g = cases.rough_terrain(20, 24, seed=2, offset=3)
    kw = cases.grid_kwargs(g)
    in0, in1 = kw["vec_norm"].shape[:2]
    return kw, in0, in1


# ---- Python ------------------------------------------------------------------------------------------------------

def test_signatures_and_defaults():
    sig = inspect.signature(horizon.horizon_distance)
    names = list(sig.parameters)
    assert names == ["vert_grid", "dem_dim_0", "dem_dim_1", "vec_norm", "vec_north", "offset_0", "offset_1", "hori", "dist_search",
                     "hori_acc", "geom_type", "vert_simp", "num_vert_simp", "tri_ind_simp", "num_tri_simp", "elev_ang_low_lim",
                     "mask", "ray_org_elev", "device", "scene", "layout", "rows", "_chunk_rows"]
    defaults = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    for n in ("vert_simp", "tri_ind_simp"):
        ours, theirs = defaults.pop(n), inspect.signature(horizon.horizon_gridded).parameters[n].default
        assert ours.dtype == theirs.dtype and np.array_equal(ours, theirs)
    assert defaults == dict(hori_acc=0.25, geom_type="grid", num_vert_simp=1, num_tri_simp=1, elev_ang_low_lim=-15.0, mask=None,
                            ray_org_elev=0.01, device=0, scene=None, layout="cell_major", rows=None, _chunk_rows=0)
    for n in names:
        kind = sig.parameters[n].kind
        assert kind is (inspect.Parameter.KEYWORD_ONLY if names.index(n) >= names.index("device")
                        else inspect.Parameter.POSITIONAL_OR_KEYWORD), n
    g = list(inspect.signature(horizon.horizon_gridded).parameters)
    p = inspect.signature(horizon.horizon_gridded).parameters["hori_dist"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert g[g.index("hori_dtype") + 1] == "hori_dist"
    import horayzon
    assert horayzon.horizon.horizon_distance is horizon.horizon_distance
    assert "lower ridge" in horizon.horizon_distance.__doc__       # the docstring says which ridge is reported


def test_horizon_distance_refusals(no_library):
    kw, in0, in1 = _grid()
    hori = np.zeros((in0, in1, A), np.float32)
    D = lambda **over: horizon.horizon_distance(**{**kw, "hori": hori, "dist_search": 1.0, **over})      # noqa: E731
    # dtypes and dimensions
    with pytest.raises(TypeError, match="incorrect type"):
        D(hori=hori.tolist())
    for bad in (np.float64, np.int16, np.float16, np.uint8):
        with pytest.raises(ValueError, match="dtype mismatch"):
            D(hori=hori.astype(bad))
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        D(hori=hori[:, :, 0])
    with pytest.raises(ValueError, match="dtype mismatch"):
        D(vec_norm=kw["vec_norm"].astype(np.float64))
    with pytest.raises(ValueError, match="dtype mismatch"):
        D(vert_grid=kw["vert_grid"].astype(np.float64))
    with pytest.raises(ValueError, match="int32_t"):
        D(tri_ind_simp=np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="expected 2"):
        D(mask=np.ones((in0, in1, 1), np.uint8))
    # shapes against vec_norm, in both layouts
    for shape in ((in0 + 1, in1, A), (in0, in1 - 1, A), (A, in0, in1)):
        with pytest.raises(ValueError, match="shape of 'hori'"):
            D(hori=np.zeros(shape, np.float32))
    for shape in ((A, in0 + 1, in1), (in0, in1, A)):
        with pytest.raises(ValueError, match="shape of 'hori'"):
            D(hori=np.zeros(shape, np.float32), layout="azim_major")
    with pytest.raises(ValueError, match="vec_norm and/or vec_north"):
        D(vec_north=kw["vec_north"][1:])
    with pytest.raises(ValueError, match="offset_0, offset_1 and vec_norm"):
        D(offset_0=kw["offset_0"] + 4)
    with pytest.raises(ValueError, match="vert_grid, dem_dim_0 and dem_dim_1"):
        D(dem_dim_0=kw["dem_dim_0"] + 5)
    with pytest.raises(ValueError, match="shape of mask"):
        D(mask=np.ones((in0, in1 + 1), np.uint8))
    with pytest.raises(TypeError, match="'uint8'"):
        D(mask=np.ones((in0, in1), np.int32))
    # layout, rows and the scalars
    for bad in ("planes", "", None, 1):
        with pytest.raises(ValueError, match="unknown 'layout'"):
            D(layout=bad)
    for bad in ((0, 0), (3, 2), (-1, 4), (0, in0 + 1), (1, 2, 3)):
        with pytest.raises(ValueError, match="'rows' must be"):
            D(rows=bad)
    with pytest.raises(TypeError, match="0.005 m"):
        D(ray_org_elev=0.004)
    with pytest.raises(ValueError, match="10 degree"):
        D(hori_acc=10.5)
    with pytest.raises(ValueError, match="geom_type"):
        D(geom_type="mesh")
    big = 32768
    with pytest.raises(ValueError, match="32'767"):
        D(vert_grid=np.zeros(3 * big * 24, np.float32), dem_dim_0=big)


def test_hori_dist_refusals(no_library):
    kw, in0, in1 = _grid()
    tilt = np.zeros(kw["vec_norm"].shape, np.float32)
    tilt[..., 2] = 1.0
    for extra in (dict(topo=("openness",), topo_only=True), dict(svf_vec_tilt=tilt, svf_only=True)):
        for dtype in horizon.HORI_DTYPES:
            with pytest.raises(ValueError, match="no horizon to"):
                horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=A, hori_dist=True, hori_dtype=dtype, **extra)
    # the reference's checks still come first
    with pytest.raises(ValueError, match="ray_algorithm"):
        horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=A, hori_dist=True, topo=("openness",), topo_only=True,
                                ray_algorithm="fast")


def test_which_entry_point_is_reached(monkeypatch):
    """Without hori_dist every call reaches the library exactly as before; with it the _dist forms get the kind of the
    horizon and the distance buffer behind it."""
    kw, in0, in1 = _grid()
    reached = []

    class Lib:
        def __getattr__(self, name):
            def f(*a):
                reached.append((name, a))
                return 0
            return f
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    scene = type("S", (), dict(_h=1, device=0))()
    tilt = np.zeros(kw["vec_norm"].shape, np.float32)
    for with_scene, base in ((False, 25), (True, 18)):
        sc = dict(scene=scene) if with_scene else {}
        sfx = "_scene" if with_scene else ""
        before = (("hz_horizon_gridded" + sfx, {}, base), ("hz_horizon_gridded%s_planes" % sfx, dict(layout="azim_major"), base + 1),
                  ("hz_horizon_gridded%s_q16" % sfx, dict(hori_dtype="uint16"), base + 2),
                  ("hz_horizon_gridded%s_ex" % sfx, dict(topo=("openness", "svf"), topo_vec_tilt=tilt), base + 1))
        for name, extra, n in before:
            for flag in ({}, dict(hori_dist=False)):
                horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=A, **extra, **sc, **flag)
                assert reached[-1][0] == name and len(reached[-1][1]) == n, (name, flag)
        at = 5 if with_scene else 7
        for layout, planes in (("cell_major", 0), ("azim_major", 1)):
            for dtype, u16 in (("float32", 0), ("uint16", 2)):
                out = horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=A, layout=layout, hori_dtype=dtype, rows=(2, 5),
                                              hori_dist=True, **sc)
                name, a = reached[-1]
                assert name == "hz_horizon_gridded%s_dist" % sfx and len(a) == base + 3
                hori, dist, azim = out
                assert (a[at], a[at + 1], a[at + 2]) == (hori.ctypes.data, planes | u16, dist.ctypes.data)
                assert a[at + 3:at + 6] == (in0, in1, A)
                assert dist.dtype == np.float32 and dist.shape == hori.shape == ((A, in0, in1) if planes else (in0, in1, A))
                assert np.isnan(dist).all() and azim.shape == (A,)      # pre-filled: the stub wrote nothing
        out = horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=A, hori_dist=True, topo=("openness",), **sc)
        assert len(out) == 4 and set(out[3]) == {"openness"} and out[2].shape == (A,)
    # the stand-alone call
    hori = np.zeros((in0, in1, A), np.uint16)
    d = horizon.horizon_distance(**kw, hori=hori, dist_search=1.0)
    name, a = reached[-1]
    assert name == "hz_horizon_distance" and len(a) == 25 and a[4] == 2 and a[5] == d.ctypes.data and a[12] == A
    d = horizon.horizon_distance(**kw, hori=np.zeros((A, in0, in1), np.float32), dist_search=1.0, layout="azim_major", scene=scene)
    name, a = reached[-1]
    assert name == "hz_horizon_distance_scene" and len(a) == 18 and a[2] == 1 and a[10] == A and d.shape == (A, in0, in1)


# ---- C -----------------------------------------------------------------------------------------------------------

def test_declarations_exports_and_documents():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for name in NEW:
        assert re.search(r"int %s\(" % name, flat), name
    assert "#define HZ_HORI_PLANES 1" in hdr and "#define HZ_HORI_U16 2" in hdr
    assert (_lib.HORI_PLANES, _lib.HORI_U16) == (1, 2)
    L = _lib.lib()
    for name, n_args in zip(NEW, (25, 18, 28, 21)):
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args, name
    # the _dist forms are the _ex forms with `int hori_kind, float *dist_buffer` behind the horizon
    for name in ("hz_horizon_gridded", "hz_horizon_gridded_scene"):
        ex = re.search(r"int %s_ex\((.*?)\);" % name, flat).group(1)
        d = re.search(r"int %s_dist\((.*?)\);" % name, flat).group(1)
        assert d == ex.replace("float *hori_buffer", "void *hori, int hori_kind, float *dist_buffer"), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, name


def test_abi_revision_and_struct_sizes_are_unchanged():
    L = _lib.lib()
    assert L.hz_abi_version() == 6
    a, b = C.c_int(0), C.c_int(0)
    assert L.hz_abi_struct_sizes(C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (C.sizeof(_lib.hz_opts), C.sizeof(_lib.hz_stats)) == (96, 232)


def test_c_entry_points_check_their_arguments():
    """NULL pointers, kinds out of range, odd addresses and non-positive lengths: HZ_ERR_ARG (1) and a message, before any
    device is touched."""
    L = _lib.lib()
    err = lambda: L.hz_last_error() or b""      # noqa: E731
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    o = _lib.hz_opts()
    one_shot = lambda h, kind, d, d0, d1, a: L.hz_horizon_gridded_dist(      # noqa: E731
        p, 4, 4, p, p, 0, 0, h, kind, d, d0, d1, a, 1.0, 0.25, b"guess_constant", b"grid", p, 1, p, 1, -15.0, p, 0.0, 0.01,
        C.byref(o), None, None)
    assert one_shot(None, 0, p, 2, 2, 2) == 1 and b"hori is NULL" in err()
    assert one_shot(p, 0, None, 2, 2, 2) == 1 and b"dist_buffer is NULL" in err()
    for kind in (-1, 4):
        assert one_shot(p, kind, p, 2, 2, 2) == 1 and b"hori_kind" in err()
    assert one_shot(p + 1, 2, p, 2, 2, 2) == 1 and b"aligned" in err()
    for lens in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert one_shot(p, 1, p, *lens) == 1 and b"must be positive" in err(), lens
    o.skip_hori = 1
    assert one_shot(p, 0, p, 2, 2, 2) == 1 and b"no horizon" in err()
    assert L.hz_horizon_gridded_scene_dist(None, p, p, 0, 0, p, 0, p, 2, 2, 2, 1.0, 0.25, b"guess_constant", -15.0, p, 0.0, 0.01,
                                           None, None, None) == 1 and b"scene is NULL" in err()
    assert L.hz_horizon_distance_scene(None, p, 0, p, p, p, 0, 0, 2, 2, 2, 1.0, 0.25, -15.0, p, 0.01, None, None) == 1
    assert b"scene is NULL" in err()
    assert L.hz_horizon_distance(p, 4, 4, None, 0, p, p, p, 0, 0, 2, 2, 2, 1.0, 0.25, b"grid", p, 1, p, 1, -15.0, p, 0.01,
                                 None, None) == 1 and b"NULL" in err()
    for v in (16, 32, 64, -1):
        assert L.hz_debug_set(b"horidist_block_w", v) == 0
    assert L.hz_debug_set(b"horidist_block_w", 12) == 1 and b"horidist_block_w" in err()
