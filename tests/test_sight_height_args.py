"""Terrain.sight_height (hz_terrain_sight_height) and sight_heights: argument checks, the declaration and the export.  No GPU
needed: every check here fires before anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import Terrain, sight_heights
from tests.terrain_args import _terrain, no_library  # noqa: F401 -- pytest finds the fixture in this namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
S = 5


def _obs(n=S):
    return np.ones((n, 3), np.float32)


def _tab(*values, dtype=np.float32):
    return np.array(values or (0.05, 1.0, 2.5), dtype)


def _height(n=S, shape=SHAPE, dtype=np.float32):
    return np.zeros((n,) + shape, dtype)


def _lowest(shape=SHAPE, dtype=np.float32):
    return np.zeros(shape, dtype)


def _cells(n=S, dtype=np.int64):
    return np.zeros(n, dtype)


def _bad_obs(value):
    o = _obs()
    o[3, 1] = value
    return o


BAD_CALLS = [
    # (arguments, exception class, message pattern)
    (lambda: ((_obs().tolist(), _tab()), dict(lowest=_lowest())), TypeError, "observers"),
    (lambda: ((_obs().astype(np.float64), _tab()), dict(lowest=_lowest())), ValueError, "dtype"),
    (lambda: ((_obs()[0], _tab()), dict(lowest=_lowest())), ValueError, "dimensions"),
    (lambda: ((np.ones((S, 4), np.float32), _tab()), dict(lowest=_lowest())), ValueError, "observers"),
    (lambda: ((np.ones((0, 3), np.float32), _tab()), dict(lowest=_lowest())), ValueError, "observers"),
    (lambda: ((np.ones((3, S), np.float32).T, _tab()), dict(lowest=_lowest())), ValueError, "C-contiguous"),
    (lambda: ((_bad_obs(np.nan), _tab()), dict(lowest=_lowest())), ValueError, "non-finite"),
    (lambda: ((_bad_obs(np.inf), _tab()), dict(cells_reached=_cells())), ValueError, "non-finite"),
    # the table
    (lambda: ((_obs(), [0.05, 1.0]), dict(lowest=_lowest())), TypeError, "heights"),
    (lambda: ((_obs(), 0.05), dict(lowest=_lowest())), TypeError, "heights"),
    (lambda: ((_obs(), None), dict(lowest=_lowest())), TypeError, "heights"),
    (lambda: ((_obs(), _tab(dtype=np.float64)), dict(lowest=_lowest())), ValueError, "dtype"),
    (lambda: ((_obs(), _tab().reshape(1, 3)), dict(lowest=_lowest())), ValueError, "dimensions"),
    (lambda: ((_obs(), np.zeros(0, np.float32)), dict(lowest=_lowest())), ValueError, "1 to 65535"),
    (lambda: ((_obs(), np.arange(1, 65537, dtype=np.float32)), dict(lowest=_lowest())), ValueError, "1 to 65535"),
    (lambda: ((_obs(), np.arange(1, 7, dtype=np.float32)[::2]), dict(lowest=_lowest())), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _tab(0.05, np.nan, 2.0)), dict(lowest=_lowest())), ValueError, "non-finite"),
    (lambda: ((_obs(), _tab(0.05, 1.0, np.inf)), dict(lowest=_lowest())), ValueError, "non-finite"),
    (lambda: ((_obs(), _tab(0.004, 1.0)), dict(lowest=_lowest())), ValueError, "0.005"),
    (lambda: ((_obs(), _tab(0.0, 1.0)), dict(lowest=_lowest())), ValueError, "0.005"),
    (lambda: ((_obs(), _tab(-1.0)), dict(lowest=_lowest())), ValueError, "0.005"),
    (lambda: ((_obs(), _tab(0.05, 1.0, 1.0)), dict(lowest=_lowest())), ValueError, "strictly increasing"),
    (lambda: ((_obs(), _tab(0.05, 2.0, 1.0)), dict(lowest=_lowest())), ValueError, "strictly increasing"),
    # the outputs
    (lambda: ((_obs(), _tab()), dict()), ValueError, "at least one"),
    (lambda: ((_obs(), _tab()), dict(height=None, lowest=None, cells_reached=None)), ValueError, "at least one"),
    (lambda: ((_obs(), _tab()), dict(height=_height(S - 1))), ValueError, "'height' has incorrect shape"),
    (lambda: ((_obs(), _tab()), dict(height=_height(shape=(6, 8)))), ValueError, "incorrect shape"),
    (lambda: ((_obs(), _tab()), dict(height=_height(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_obs(), _tab()), dict(height=_height()[0])), ValueError, "dimensions"),
    (lambda: ((_obs(), _tab()), dict(height=_height().tolist())), TypeError, "height"),
    (lambda: ((_obs(), _tab()), dict(height=_height(shape=SHAPE[::-1]).transpose(0, 2, 1))), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest((7, 6)))), ValueError, "incorrect shape"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(dtype=np.int32))), ValueError, "dtype"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest((1,) + SHAPE))), ValueError, "dimensions"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(SHAPE[::-1]).T)), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _tab()), dict(cells_reached=_cells(S + 1))), ValueError, "'cells_reached' has incorrect shape"),
    (lambda: ((_obs(), _tab()), dict(cells_reached=_cells(dtype=np.int32))), ValueError, "dtype"),
    (lambda: ((_obs(), _tab()), dict(cells_reached=_cells(2 * S)[::2])), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _tab()), dict(cells_reached=_cells().reshape(S, 1))), ValueError, "dimensions"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(), max_dist=0.0)), ValueError, "max_dist"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(), max_dist=-5.0)), ValueError, "max_dist"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(), max_dist=np.nan)), ValueError, "max_dist"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(), max_dist=1e-60)), ValueError, "max_dist"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(), max_dist="far")), TypeError, "max_dist"),
    (lambda: ((_obs(), _tab()), dict(lowest=_lowest(), max_dist=False)), TypeError, "max_dist"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_invalid_arguments_raise_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().sight_height(*args, **kw)


def test_one_array_for_two_outputs(no_library):
    same = _lowest((1,) + SHAPE)
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().sight_height(_obs(1), _tab(), height=same, lowest=same[0])
    raw = np.zeros(S * 8, np.uint8)
    with pytest.raises(ValueError, match="different arrays"):
        _terrain((2, 5)).sight_height(_obs(), _tab(), lowest=raw.view(np.float32).reshape(2, 5), cells_reached=raw.view(np.int64))


def test_torch_tensors_must_be_on_the_terrains_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().sight_height(_obs(), _tab(), lowest=torch.zeros(SHAPE, dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().sight_height(_obs(), _tab(), height=torch.zeros((S,) + SHAPE, dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().sight_height(_obs(), _tab(), cells_reached=torch.zeros(S, dtype=torch.int64))
    with pytest.raises(ValueError, match="device"):
        _terrain().sight_height(torch.ones((S, 3), dtype=torch.float32), _tab(), lowest=_lowest())
    with pytest.raises(ValueError, match="dtype"):
        _terrain().sight_height(_obs(), _tab(), lowest=torch.zeros(SHAPE, dtype=torch.int32))
    with pytest.raises(TypeError, match="heights"):
        _terrain().sight_height(_obs(), torch.ones(3, dtype=torch.float32), lowest=_lowest())


def test_uninitialised_terrain(no_library):
    t = _terrain()
    t._shape = None
    for kw in (dict(lowest=_lowest()), dict(height=_height()), dict(cells_reached=_cells())):
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            t.sight_height(_obs(), _tab(), **kw)


def test_signature():
    params = inspect.signature(Terrain.sight_height).parameters
    assert list(params) == ["self", "observers", "heights", "height", "lowest", "cells_reached", "max_dist"]
    for name in list(params)[3:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None
    params = inspect.signature(sight_heights).parameters
    assert list(params) == ["height_max", "height_acc", "height_min"]
    assert params["height_acc"].default == 0.25 and params["height_min"].default == 0.05


def test_outputs_are_keyword_only(no_library):
    with pytest.raises(TypeError):
        _terrain().sight_height(_obs(), _tab(), _height())


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.Terrain.sight_height is Terrain.sight_height
    assert horayzon.shadow.sight_heights is sight_heights


def test_horizon_terrain_has_no_sight_height():
    from horayzon_amd.shadow import HorizonTerrain
    assert not hasattr(HorizonTerrain, "sight_height")


# --- sight_heights -----------------------------------------------------------------------------------------------------

def test_sight_heights_is_the_documented_expression():
    for height_max, acc, lo in ((256.05, 2.0, 0.05), (256.05, 0.25, 0.05), (100.0, 0.3, 0.05), (10.0, 0.25, 1.0), (0.05, 0.25, 0.05),
                                (50.0, 0.7, 0.005)):
        k = int(np.ceil((np.float64(height_max) - np.float64(lo)) / np.float64(acc)))
        want = (np.float64(lo) + np.arange(k + 1) * np.float64(acc)).astype(np.float32)
        got = sight_heights(height_max, acc, lo)
        assert got.dtype == np.float32 and got.ndim == 1 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[1:] > got[:-1]).all() and got[0] == np.float32(lo)
        # the last entry is the first at or above height_max
        assert np.float64(lo) + k * np.float64(acc) >= height_max and (k == 0 or np.float64(lo) + (k - 1) * np.float64(acc) < height_max)
    assert sight_heights(256.05, 2.0).size == 129 and sight_heights(256.05).size == 1025
    assert sight_heights(0.05).tolist() == [np.float32(0.05)]
    assert sight_heights(10, 1, 1).tolist() == [float(v) for v in range(1, 11)]


def test_sight_heights_limits():
    assert sight_heights(0.05 + 65534 * 0.25 - 0.1, 0.25).size == 65535
    with pytest.raises(ValueError, match="65535"):
        sight_heights(0.05 + 65535 * 0.25 - 0.1, 0.25)
    with pytest.raises(ValueError, match="65535"):
        sight_heights(1e9, 0.25)
    # a step below the spacing of float32 near the top of the table: neighbours round to the same number
    with pytest.raises(ValueError, match="equal"):
        sight_heights(4096.01, 0.0625 / 512, 4095.9)
    for bad in (dict(height_acc=0.0), dict(height_acc=-1.0), dict(height_min=0.004), dict(height_min=0.0), dict(height_min=-2.0),
                dict(height_min=300.0), dict(height_acc=np.nan), dict(height_min=np.inf)):
        with pytest.raises(ValueError):
            sight_heights(256.05, **bad)
    with pytest.raises(ValueError):
        sight_heights(np.inf)
    for bad in ("10", None, True, [1.0]):
        with pytest.raises(TypeError):
            sight_heights(bad)
    with pytest.raises(TypeError):
        sight_heights(10.0, height_acc="0.25")


def test_a_table_of_sight_heights_passes_the_checks_of_sight_height(no_library):
    """... up to the point where the library would be called: the loader replaced by `no_library` raises AssertionError there."""
    with pytest.raises(AssertionError, match="the library was called"):
        _terrain().sight_height(_obs(), sight_heights(256.05), lowest=_lowest())
    no_library.clear()


# --- the C side --------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    decl = re.search(r"int hz_terrain_sight_height\((.*?)\);", hdr, flags=re.S)
    assert decl, "hz_terrain_sight_height is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["hz_terrain *terrain", "const float *observers", "int num_obs", "const float *heights", "int num_heights",
                      "float max_dist", "float *height", "float *lowest", "int64_t *cells_reached", "hz_stats *stats"]
    assert "hz_terrain_sight_height" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "hz_terrain_sight_height")
    assert len(L.hz_terrain_sight_height.argtypes) == 10


def test_abi_revision_and_structs_are_unchanged():
    """An added entry point: no struct grows, the revision stays."""
    import ctypes as C
    L = _lib.lib()
    assert L.hz_abi_version() == 6
    opts, stats = C.c_int(0), C.c_int(0)
    assert L.hz_abi_struct_sizes(C.byref(opts), C.byref(stats)) == 0
    assert stats.value == C.sizeof(_lib.hz_stats)


def test_c_entry_point_checks_its_arguments():
    """The C entry point's own checks, before any device is touched."""
    L = _lib.lib()
    obs, tab, low = _obs(), _tab(), _lowest()
    assert L.hz_terrain_sight_height(None, obs.ctypes.data, S, tab.ctypes.data, 3, 0.0, None, low.ctypes.data, None, None) == 1
    assert b"not initialised" in L.hz_last_error()
