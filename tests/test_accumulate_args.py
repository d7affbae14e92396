"""Terrain.accumulate (hz_terrain_accumulate): argument checks, the declaration and the export.  No GPU needed: every check
here fires before anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import Terrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)


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
    """A Terrain that looks initialised to the Python checks, without a device behind it."""
    t = Terrain.__new__(Terrain)
    t._h = None
    t._shape = shape
    t.device = 0
    t.last_stats = None
    return t


def _sun(n=5):
    return np.ones((n, 3), np.float32)


def _out(shape=SHAPE, dtype=np.float32):
    return np.zeros(shape, dtype)


BAD_CALLS = [
    # (arguments, exception class, message pattern)
    (lambda: ((_sun().tolist(),), dict(sunlit_sum=_out())), TypeError, "sun_positions"),
    (lambda: ((_sun().astype(np.float64),), dict(sunlit_sum=_out())), ValueError, "dtype"),
    (lambda: ((_sun()[0],), dict(sunlit_sum=_out())), ValueError, "dimensions"),
    (lambda: ((np.ones((5, 4), np.float32),), dict(sunlit_sum=_out())), ValueError, "sun_positions"),
    (lambda: ((np.ones((0, 3), np.float32),), dict(sunlit_sum=_out())), ValueError, "sun_positions"),
    (lambda: ((np.ones((3, 5), np.float32).T,), dict(sunlit_sum=_out())), ValueError, "C-contiguous"),
    (lambda: ((_sun(), np.ones(4, np.float32)), dict(sunlit_sum=_out())), ValueError, "weights"),
    (lambda: ((_sun(), np.ones(6, np.float32)), dict(sunlit_sum=_out())), ValueError, "weights"),
    (lambda: ((_sun(), np.ones(5, np.float64)), dict(sunlit_sum=_out())), ValueError, "dtype"),
    (lambda: ((_sun(), np.ones((5, 1), np.float32)), dict(sunlit_sum=_out())), ValueError, "dimensions"),
    (lambda: ((_sun(), [1.0] * 5), dict(sunlit_sum=_out())), TypeError, "weights"),
    (lambda: ((_sun(), np.ones(10, np.float32)[::2]), dict(sunlit_sum=_out())), ValueError, "C-contiguous"),
    (lambda: ((_sun(),), dict()), ValueError, "at least one"),
    (lambda: ((_sun(),), dict(sw_dir_cor_sum=None, sunlit_sum=None)), ValueError, "at least one"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out((6, 8)))), ValueError, "incorrect shape"),
    (lambda: ((_sun(),), dict(sw_dir_cor_sum=_out((7, 6)))), ValueError, "incorrect shape"),
    (lambda: ((_sun(),), dict(sw_dir_cor_sum=_out(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out(dtype=np.uint8))), ValueError, "dtype"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out((1,) + SHAPE))), ValueError, "dimensions"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out(SHAPE[::-1]).T)), ValueError, "C-contiguous"),
    (lambda: ((_sun(),), dict(sunlit_sum=_out().tolist())), TypeError, "sunlit_sum"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_invalid_arguments_raise_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().accumulate(*args, **kw)


def test_one_array_for_both_outputs(no_library):
    out = _out()
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().accumulate(_sun(), sw_dir_cor_sum=out, sunlit_sum=out)


def test_torch_tensors_must_be_on_the_terrains_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().accumulate(_sun(), sunlit_sum=torch.zeros(SHAPE, dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().accumulate(torch.ones((5, 3), dtype=torch.float32), sunlit_sum=_out())
    with pytest.raises(ValueError, match="device"):
        _terrain().accumulate(_sun(), torch.ones(5, dtype=torch.float32), sunlit_sum=_out())
    with pytest.raises(ValueError, match="dtype"):
        _terrain().accumulate(_sun(), sunlit_sum=torch.zeros(SHAPE, dtype=torch.float64))


def test_uninitialised_terrain(no_library):
    t = _terrain()
    t._shape = None
    with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
        t.accumulate(_sun(), sunlit_sum=_out())


def test_outputs_are_keyword_only(no_library):
    params = inspect.signature(Terrain.accumulate).parameters
    assert params["sw_dir_cor_sum"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["sunlit_sum"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["weights"].default is None
    with pytest.raises(TypeError):
        _terrain().accumulate(_sun(), None, _out())


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.Terrain.accumulate is Terrain.accumulate


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    decl = re.search(r"int hz_terrain_accumulate\((.*?)\);", hdr, flags=re.S)
    assert decl, "hz_terrain_accumulate is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert params == ["hz_terrain *terrain", "const float *sun_positions", "const float *weights", "int num_sun",
                      "float *sw_dir_cor_sum", "float *sunlit_sum", "hz_stats *stats"]
    assert "hz_terrain_accumulate" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "hz_terrain_accumulate")
    assert len(L.hz_terrain_accumulate.argtypes) == 7


def test_c_entry_point_checks_its_arguments():
    """The C entry point's own checks, before any device is touched."""
    L = _lib.lib()
    sun = _sun()
    out = _out()
    assert L.hz_terrain_accumulate(None, sun.ctypes.data, None, 5, None, out.ctypes.data, None) == 1
    assert b"not initialised" in L.hz_last_error()


def test_accum_chunk_knob_is_accepted():
    L = _lib.lib()
    for v in (1, 3, 7, -1):
        assert L.hz_debug_set(b"accum_chunk", v) == 0
    assert L.hz_debug_set(b"accum_chunk_typo", 1) != 0
