"""HorizonTerrain.sw_dir_cor_coarse (hz_horizon_terrain_sw_dir_cor_coarse): argument checks, the declaration and the export,
as tests/test_coarse_args.py has them for Terrain.sw_dir_cor_coarse -- the same classes, messages and order.  No GPU needed:
every check here fires before anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import HorizonTerrain, Terrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 8)
S = 5


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


def _sun(n=S):
    return np.ones((n, 3), np.float32)


def _out(P=2, n=S, dtype=np.float32):
    """An output of the right shape for pixel_per_gc = P (an int or a pair)."""
    P0, P1 = (P, P) if isinstance(P, int) else P
    return np.zeros((n, SHAPE[0] // P0, SHAPE[1] // P1), dtype)


BAD_CALLS = [
    # (arguments, exception class, message pattern)
    (lambda: ((_sun().tolist(), 2), dict(f_cor=_out())), TypeError, "sun_positions"),
    (lambda: ((_sun().astype(np.float64), 2), dict(f_cor=_out())), ValueError, "dtype"),
    (lambda: ((_sun()[0], 2), dict(f_cor=_out())), ValueError, "dimensions"),
    (lambda: ((np.ones((S, 4), np.float32), 2), dict(f_cor=_out())), ValueError, "sun_positions"),
    (lambda: ((np.ones((0, 3), np.float32), 2), dict(f_cor=_out(n=0))), ValueError, "sun_positions"),
    (lambda: ((np.ones((3, S), np.float32).T, 2), dict(f_cor=_out())), ValueError, "C-contiguous"),
    # pixel_per_gc: values
    (lambda: ((_sun(), 0), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),
    (lambda: ((_sun(), -1), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),
    (lambda: ((_sun(), 4), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),            # 4 does not divide 6
    (lambda: ((_sun(), (2, 3)), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),       # 3 does not divide 8
    (lambda: ((_sun(), (7, 1)), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),       # 7 > 6
    (lambda: ((_sun(), (2, 16)), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),
    (lambda: ((_sun(), (0, 2)), dict(f_cor=_out())), ValueError, r"pixel_per_gc.*\(6, 8\)"),
    # pixel_per_gc: types
    (lambda: ((_sun(), 2.0), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), True), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), (2,)), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), (2, 2, 2)), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), (2, 2.0)), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), (True, 2)), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), None), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    (lambda: ((_sun(), "2"), dict(f_cor=_out())), TypeError, "pixel_per_gc"),
    # outputs
    (lambda: ((_sun(), 2), dict()), ValueError, "at least one"),
    (lambda: ((_sun(), 2), dict(f_cor=None, sunlit_frac=None)), ValueError, "at least one"),
    (lambda: ((_sun(), 2), dict(f_cor=_out((3, 2)))), ValueError, "'f_cor' has incorrect shape"),
    (lambda: ((_sun(), (3, 2)), dict(sunlit_frac=_out(2))), ValueError, "'sunlit_frac' has incorrect shape"),
    (lambda: ((_sun(), 2), dict(f_cor=_out(), sunlit_frac=_out(1))), ValueError, "'sunlit_frac' has incorrect shape"),
    (lambda: ((_sun(), 2), dict(f_cor=_out(n=S + 1))), ValueError, "'f_cor' has incorrect shape"),
    (lambda: ((_sun(), 2), dict(f_cor=_out()[0])), ValueError, "dimensions"),
    (lambda: ((_sun(), 2), dict(f_cor=_out(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_sun(), 2), dict(sunlit_frac=_out(dtype=np.uint8))), ValueError, "dtype"),
    (lambda: ((_sun(), 2), dict(f_cor=np.zeros((S, 4, 3), np.float32).transpose(0, 2, 1))), ValueError, "C-contiguous"),
    (lambda: ((_sun(), 2), dict(sunlit_frac=np.zeros((S, 3, 8), np.float32)[:, :, ::2])), ValueError, "C-contiguous"),
    (lambda: ((_sun(), 2), dict(f_cor=_out().tolist())), TypeError, "f_cor"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_invalid_arguments_raise_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().sw_dir_cor_coarse(*args, **kw)


def test_one_array_for_both_outputs(no_library):
    out = _out()
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().sw_dir_cor_coarse(_sun(), 2, f_cor=out, sunlit_frac=out)


def test_torch_tensors_must_be_on_the_terrains_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().sw_dir_cor_coarse(_sun(), 2, f_cor=torch.zeros((S, 3, 4), dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().sw_dir_cor_coarse(torch.ones((S, 3), dtype=torch.float32), 2, f_cor=_out())
    with pytest.raises(ValueError, match="dtype"):
        _terrain().sw_dir_cor_coarse(_sun(), 2, sunlit_frac=torch.zeros((S, 3, 4), dtype=torch.float64))


def test_uninitialised_terrain(no_library):
    t = _terrain()
    t._shape = None
    with pytest.raises(_lib.HorayzonHipError, match="HorizonTerrain is not initialised"):
        t.sw_dir_cor_coarse(_sun(), 2, f_cor=_out())


def test_outputs_are_keyword_only(no_library):
    params = inspect.signature(HorizonTerrain.sw_dir_cor_coarse).parameters
    assert list(params)[1:3] == ["sun_positions", "pixel_per_gc"]
    assert params["f_cor"].kind is inspect.Parameter.KEYWORD_ONLY and params["f_cor"].default is None
    assert params["sunlit_frac"].kind is inspect.Parameter.KEYWORD_ONLY and params["sunlit_frac"].default is None
    with pytest.raises(TypeError):
        _terrain().sw_dir_cor_coarse(_sun(), 2, _out())


def test_numpy_integers_are_integers(no_library):
    """np.int64 pixel counts (what shape arithmetic yields) pass the type check: the first failure is a later rule."""
    with pytest.raises(ValueError, match="different arrays"):
        out = _out((2, 4))
        _terrain().sw_dir_cor_coarse(_sun(), (np.int64(2), np.int32(4)), f_cor=out, sunlit_frac=out)


def test_signature_is_terrains():
    assert str(inspect.signature(HorizonTerrain.sw_dir_cor_coarse)) == str(inspect.signature(Terrain.sw_dir_cor_coarse))


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_messages_are_terrains(no_library, make, exc, pattern):
    """The same bad call on a Terrain and on a HorizonTerrain: the same class and the same text."""
    tr = Terrain.__new__(Terrain)
    tr._h, tr._shape, tr.device, tr.last_stats = None, SHAPE, 0, None
    msgs = []
    for t in (tr, _terrain()):
        args, kw = make()
        with pytest.raises(exc) as e:
            t.sw_dir_cor_coarse(*args, **kw)
        msgs.append((type(e.value), str(e.value)))
    assert msgs[0] == msgs[1]


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.HorizonTerrain.sw_dir_cor_coarse is HorizonTerrain.sw_dir_cor_coarse


def test_header_declares_and_bindings_match():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    decl = re.search(r"int hz_horizon_terrain_sw_dir_cor_coarse\((.*?)\);", hdr, flags=re.S)
    assert decl, "hz_horizon_terrain_sw_dir_cor_coarse is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["hz_horizon_terrain *t", "const float *sun_positions", "int num_sun", "int pixel_per_gc_0",
                      "int pixel_per_gc_1", "float *f_cor", "float *sunlit_frac", "hz_stats *stats"]
    assert "hz_horizon_terrain_sw_dir_cor_coarse" in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "horayzon_amd", "_lib.py")).read()
    bound = re.search(r"L\.hz_horizon_terrain_sw_dir_cor_coarse\.argtypes = \[(.*?)\]", src)
    assert bound, "hz_horizon_terrain_sw_dir_cor_coarse has no argtypes in _lib.py"
    assert [a.strip() for a in bound.group(1).split(",")] == ["vp", "vp", "ip", "ip", "ip", "vp", "vp", "C.POINTER(hz_stats)"]


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhorayzon_hip.so is not built")
    return _lib.lib()


def test_library_exports():
    import ctypes as C
    L = _library()
    assert hasattr(L, "hz_horizon_terrain_sw_dir_cor_coarse")
    assert L.hz_horizon_terrain_sw_dir_cor_coarse.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                               C.c_void_p, C.POINTER(_lib.hz_stats)]
    assert L.hz_abi_version() == 6


def test_c_entry_point_checks_its_arguments():
    """The C entry point's own checks, before any device is touched."""
    L = _library()
    sun, out = _sun(), _out()
    assert L.hz_horizon_terrain_sw_dir_cor_coarse(None, sun.ctypes.data, S, 2, 2, out.ctypes.data, None, None) == 1
    assert b"not initialised" in L.hz_last_error()


def test_knobs_are_accepted():
    L = _library()
    for v in (256, 64, 7, -1):
        assert L.hz_debug_set(b"horisun_coarse_tile", v) == 0
    for v in (1, 0, -1):
        assert L.hz_debug_set(b"horisun_coarse_route", v) == 0
