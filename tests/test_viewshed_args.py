"""Terrain.viewshed (hz_terrain_viewshed): argument checks, the declaration and the export.  No GPU needed: every check
here fires before anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import Terrain
from tests.terrain_args import _terrain, no_library  # noqa: F401 -- pytest finds the fixture in this namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
S = 5


def _obs(n=S):
    return np.ones((n, 3), np.float32)


def _vis(n=S, shape=SHAPE, dtype=np.uint8):
    return np.zeros((n,) + shape, dtype)


def _seen(shape=SHAPE, dtype=np.int32):
    return np.zeros(shape, dtype)


def _cells(n=S, dtype=np.int64):
    return np.zeros(n, dtype)


def _bad_obs(value):
    o = _obs()
    o[3, 1] = value
    return o


BAD_CALLS = [
    # (arguments, exception class, message pattern)
    (lambda: ((_obs().tolist(),), dict(seen_count=_seen())), TypeError, "observers"),
    (lambda: ((_obs().astype(np.float64),), dict(seen_count=_seen())), ValueError, "dtype"),
    (lambda: ((_obs()[0],), dict(seen_count=_seen())), ValueError, "dimensions"),
    (lambda: ((np.ones((S, 4), np.float32),), dict(seen_count=_seen())), ValueError, "observers"),
    (lambda: ((np.ones((0, 3), np.float32),), dict(seen_count=_seen())), ValueError, "observers"),
    (lambda: ((np.ones((3, S), np.float32).T,), dict(seen_count=_seen())), ValueError, "C-contiguous"),
    (lambda: ((_bad_obs(np.nan),), dict(seen_count=_seen())), ValueError, "non-finite"),
    (lambda: ((_bad_obs(np.inf),), dict(seen_count=_seen())), ValueError, "non-finite"),
    (lambda: ((_bad_obs(-np.inf),), dict(cells_seen=_cells())), ValueError, "non-finite"),
    (lambda: ((_obs(),), dict()), ValueError, "at least one"),
    (lambda: ((_obs(),), dict(visible=None, seen_count=None, cells_seen=None)), ValueError, "at least one"),
    (lambda: ((_obs(),), dict(visible=_vis(S - 1))), ValueError, "'visible' has incorrect shape"),
    (lambda: ((_obs(),), dict(visible=_vis(shape=(6, 8)))), ValueError, "incorrect shape"),
    (lambda: ((_obs(),), dict(visible=_vis(dtype=np.int8))), ValueError, "dtype"),
    (lambda: ((_obs(),), dict(visible=_vis()[0])), ValueError, "dimensions"),
    (lambda: ((_obs(),), dict(visible=_vis().tolist())), TypeError, "visible"),
    (lambda: ((_obs(),), dict(visible=_vis(shape=SHAPE[::-1]).transpose(0, 2, 1))), ValueError, "C-contiguous"),
    (lambda: ((_obs(),), dict(seen_count=_seen((7, 6)))), ValueError, "incorrect shape"),
    (lambda: ((_obs(),), dict(seen_count=_seen(dtype=np.int64))), ValueError, "dtype"),
    (lambda: ((_obs(),), dict(seen_count=_seen(dtype=np.uint32))), ValueError, "dtype"),
    (lambda: ((_obs(),), dict(seen_count=_seen((1,) + SHAPE))), ValueError, "dimensions"),
    (lambda: ((_obs(),), dict(seen_count=_seen(SHAPE[::-1]).T)), ValueError, "C-contiguous"),
    (lambda: ((_obs(),), dict(cells_seen=_cells(S + 1))), ValueError, "'cells_seen' has incorrect shape"),
    (lambda: ((_obs(),), dict(cells_seen=_cells(dtype=np.int32))), ValueError, "dtype"),
    (lambda: ((_obs(),), dict(cells_seen=_cells(2 * S)[::2])), ValueError, "C-contiguous"),
    (lambda: ((_obs(),), dict(cells_seen=_cells().reshape(S, 1))), ValueError, "dimensions"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=0.004)), ValueError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=0.0)), ValueError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=-1.0)), ValueError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=np.nan)), ValueError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=np.inf)), ValueError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev="0.05")), TypeError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=None)), TypeError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), target_elev=True)), TypeError, "target_elev"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), max_dist=0.0)), ValueError, "max_dist"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), max_dist=-5.0)), ValueError, "max_dist"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), max_dist=np.nan)), ValueError, "max_dist"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), max_dist=1e-60)), ValueError, "max_dist"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), max_dist="far")), TypeError, "max_dist"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), max_dist=False)), TypeError, "max_dist"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), facing=1)), TypeError, "facing"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), facing=None)), TypeError, "facing"),
    (lambda: ((_obs(),), dict(seen_count=_seen(), facing="yes")), TypeError, "facing"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_invalid_arguments_raise_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().viewshed(*args, **kw)


def test_one_array_for_two_outputs(no_library):
    """The three outputs have three element types, so one array cannot be given twice as it is; two views of one buffer can."""
    raw = np.zeros(S * 8, np.uint8)
    with pytest.raises(ValueError, match="different arrays"):
        _terrain((1, 8)).viewshed(_obs(), visible=raw.reshape(S, 1, 8), cells_seen=raw.view(np.int64))
    with pytest.raises(ValueError, match="different arrays"):
        _terrain((2, 5)).viewshed(_obs(), seen_count=raw.view(np.int32).reshape(2, 5), cells_seen=raw.view(np.int64))


def test_torch_tensors_must_be_on_the_terrains_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().viewshed(_obs(), seen_count=torch.zeros(SHAPE, dtype=torch.int32))
    with pytest.raises(ValueError, match="device"):
        _terrain().viewshed(_obs(), visible=torch.zeros((S,) + SHAPE, dtype=torch.uint8))
    with pytest.raises(ValueError, match="device"):
        _terrain().viewshed(_obs(), cells_seen=torch.zeros(S, dtype=torch.int64))
    with pytest.raises(ValueError, match="device"):
        _terrain().viewshed(torch.ones((S, 3), dtype=torch.float32), seen_count=_seen())
    with pytest.raises(ValueError, match="dtype"):
        _terrain().viewshed(_obs(), seen_count=torch.zeros(SHAPE, dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        _terrain().viewshed(_obs(), cells_seen=torch.zeros(S, dtype=torch.int32))


def test_uninitialised_terrain(no_library):
    t = _terrain()
    t._shape = None
    for kw in (dict(seen_count=_seen()), dict(visible=_vis()), dict(cells_seen=_cells())):
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            t.viewshed(_obs(), **kw)


def test_signature():
    params = inspect.signature(Terrain.viewshed).parameters
    assert list(params) == ["self", "observers", "visible", "seen_count", "cells_seen", "target_elev", "max_dist", "facing"]
    for name in list(params)[2:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["visible"].default is None and params["seen_count"].default is None and params["cells_seen"].default is None
    assert params["target_elev"].default == 0.05 and params["max_dist"].default is None and params["facing"].default is True


def test_outputs_are_keyword_only(no_library):
    with pytest.raises(TypeError):
        _terrain().viewshed(_obs(), _vis())


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.Terrain.viewshed is Terrain.viewshed


def test_horizon_terrain_has_no_viewshed():
    """A stored horizon cannot answer finite lines of sight."""
    from horayzon_amd.shadow import HorizonTerrain
    assert not hasattr(HorizonTerrain, "viewshed")


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    decl = re.search(r"int hz_terrain_viewshed\((.*?)\);", hdr, flags=re.S)
    assert decl, "hz_terrain_viewshed is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["hz_terrain *terrain", "const float *observers", "int num_obs", "float target_elev", "float max_dist",
                      "int facing", "uint8_t *visible", "int32_t *seen_count", "int64_t *cells_seen", "hz_stats *stats"]
    assert "hz_terrain_viewshed" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "hz_terrain_viewshed")
    assert len(L.hz_terrain_viewshed.argtypes) == 10


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
    obs, seen = _obs(), _seen()
    assert L.hz_terrain_viewshed(None, obs.ctypes.data, S, 0.05, 0.0, 1, None, seen.ctypes.data, None, None) == 1
    assert b"not initialised" in L.hz_last_error()
