"""Terrain.panorama (hz_terrain_panorama): argument checks, the declaration and the export.  No GPU needed: every check
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
S, A, E = 5, 7, 4


def _obs(n=S):
    return np.ones((n, 3), np.float32)


def _azim(n=A):
    return np.linspace(0.0, 6.0, n).astype(np.float32)


def _elev(n=E):
    return np.linspace(-1.5, 1.5, n).astype(np.float32)


def _dist(shape=(S, E, A), dtype=np.float32):
    return np.zeros(shape, dtype)


def _point(shape=(S, E, A, 3), dtype=np.float32):
    return np.zeros(shape, dtype)


def _hits(n=S, dtype=np.int64):
    return np.zeros(n, dtype)


def _bad(a, value, at=1):
    a = a.copy()
    a.reshape(-1)[at] = value
    return a


def _frame(axis, n=S):
    v = np.zeros((n, 3), np.float32)
    v[:, axis] = 1.0
    return v


def _wide(n):
    """n float32 angles that cost no memory: a zero-stride view (C-contiguity is checked after the pixel count)."""
    return np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(n,), strides=(0,))


HALF_PI = np.float32(np.pi / 2)

# (positional arguments after the Terrain, keywords, exception class, message pattern)
BAD_CALLS = [
    (lambda: ((_obs().tolist(), _azim(), _elev(), 100.0), dict(dist=_dist())), TypeError, "observers"),
    (lambda: ((_obs().astype(np.float64), _azim(), _elev(), 100.0), dict(dist=_dist())), ValueError, "dtype"),
    (lambda: ((_obs()[0], _azim(), _elev(), 100.0), dict(dist=_dist())), ValueError, "dimensions"),
    (lambda: ((np.ones((S, 4), np.float32), _azim(), _elev(), 100.0), dict(dist=_dist())), ValueError, "'observers' has incorrect shape"),
    (lambda: ((np.ones((0, 3), np.float32), _azim(), _elev(), 100.0), dict(hits=_hits(0))), ValueError, "'observers' has incorrect shape"),
    (lambda: ((np.ones((3, S), np.float32).T, _azim(), _elev(), 100.0), dict(dist=_dist())), ValueError, "C-contiguous"),
    (lambda: ((_bad(_obs(), np.nan), _azim(), _elev(), 100.0), dict(dist=_dist())), ValueError, "'observers' has non-finite"),
    (lambda: ((_bad(_obs(), -np.inf), _azim(), _elev(), 100.0), dict(hits=_hits())), ValueError, "'observers' has non-finite"),
    (lambda: ((_obs(), _azim().tolist(), _elev(), 100.0), dict(dist=_dist())), TypeError, "azim"),
    (lambda: ((_obs(), _azim(), 0.5, 100.0), dict(dist=_dist())), TypeError, "elev"),
    (lambda: ((_obs(), _azim().astype(np.float64), _elev(), 100.0), dict(dist=_dist())), ValueError, "dtype"),
    (lambda: ((_obs(), _azim(), _elev().astype(np.float64), 100.0), dict(dist=_dist())), ValueError, "dtype"),
    (lambda: ((_obs(), _azim()[None, :], _elev(), 100.0), dict(dist=_dist())), ValueError, "dimensions"),
    (lambda: ((_obs(), _azim(), _elev().reshape(2, 2), 100.0), dict(dist=_dist())), ValueError, "dimensions"),
    (lambda: ((_obs(), _azim(0), _elev(), 100.0), dict(hits=_hits())), ValueError, "'azim' must have at least one"),
    (lambda: ((_obs(), _azim(), _elev(0), 100.0), dict(hits=_hits())), ValueError, "'elev' must have at least one"),
    (lambda: ((_obs(), _wide(2 ** 15 + 1), _wide(2 ** 15), 100.0), dict(hits=_hits())), ValueError, r"2\*\*30"),
    (lambda: ((_obs(), _wide(2 ** 30 + 1), _elev(1), 100.0), dict(hits=_hits())), ValueError, r"2\*\*30"),
    (lambda: ((_obs(), _azim(2 * A)[::2], _elev(), 100.0), dict(dist=_dist())), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _azim(), _elev(2 * E)[::2], 100.0), dict(dist=_dist())), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _bad(_azim(), np.nan), _elev(), 100.0), dict(dist=_dist())), ValueError, "'azim' has non-finite"),
    (lambda: ((_obs(), _bad(_azim(), np.inf), _elev(), 100.0), dict(dist=_dist())), ValueError, "'azim' has non-finite"),
    (lambda: ((_obs(), _azim(), _bad(_elev(), np.nan), 100.0), dict(dist=_dist())), ValueError, "'elev' has non-finite"),
    (lambda: ((_obs(), _azim(), _bad(_elev(), -np.inf), 100.0), dict(dist=_dist())), ValueError, "'elev' has non-finite"),
    (lambda: ((_obs(), _azim(), _bad(_elev(), np.nextafter(HALF_PI, np.float32(2))), 100.0), dict(dist=_dist())), ValueError, "pi/2"),
    (lambda: ((_obs(), _azim(), _bad(_elev(), -np.nextafter(HALF_PI, np.float32(2))), 100.0), dict(dist=_dist())), ValueError, "pi/2"),
    (lambda: ((_obs(), _azim(), _bad(_elev(), 1.6), 100.0), dict(dist=_dist())), ValueError, "pi/2"),
    (lambda: ((_obs(), _azim(), _elev(), None), dict(dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), "far"), dict(dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), True), dict(dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), np.ones(1, np.float32)), dict(dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), 0.0), dict(dist=_dist())), ValueError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), -5.0), dict(dist=_dist())), ValueError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), np.nan), dict(dist=_dist())), ValueError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), np.inf), dict(dist=_dist())), ValueError, "max_dist"),
    (lambda: ((_obs(), _azim(), _elev(), 1e39), dict(dist=_dist())), ValueError, "max_dist"),        # infinite as float32
    (lambda: ((_obs(), _azim(), _elev(), 1e-60), dict(dist=_dist())), ValueError, "max_dist"),       # zero as float32
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict()), ValueError, "at least one"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=None, point=None, hits=None)), ValueError, "at least one"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=_dist((S - 1, E, A)))), ValueError, "'dist' has incorrect shape"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=_dist((S, A, E)))), ValueError, "'dist' has incorrect shape"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=_dist(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=_dist()[0])), ValueError, "dimensions"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=_dist().tolist())), TypeError, "dist"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(dist=_dist((S, A, E)).transpose(0, 2, 1))), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(point=_point((S, E, A, 4)))), ValueError, "'point' has incorrect shape"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(point=_point((S, E + 1, A, 3)))), ValueError, "'point' has incorrect shape"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(point=_point(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(point=_dist())), ValueError, "dimensions"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(point=_point((3, S, E, A)).transpose(1, 2, 3, 0))), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(point=(1, 2, 3))), TypeError, "point"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(S + 1))), ValueError, "'hits' has incorrect shape"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(dtype=np.int32))), ValueError, "dtype"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(dtype=np.uint64))), ValueError, "dtype"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(2 * S)[::2])), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits().reshape(S, 1))), ValueError, "dimensions"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1))), ValueError, "given together"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_norm=_frame(2))), ValueError, "given together"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1).tolist(), vec_norm=_frame(2))), TypeError, "vec_north"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1), vec_norm=7)), TypeError, "vec_norm"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1).astype(np.float64), vec_norm=_frame(2))), ValueError, "dtype"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1), vec_norm=_frame(2)[0])), ValueError, "dimensions"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1, S + 1), vec_norm=_frame(2))), ValueError, "shape of 'vec_north'"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1), vec_norm=np.ones((S, 2), np.float32))), ValueError, "shape of 'vec_north'"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=np.ascontiguousarray(_frame(1).T).T, vec_norm=_frame(2))), ValueError, "C-contiguous"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1) * np.float32(1.01), vec_norm=_frame(2))), ValueError, "not normalised"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1), vec_norm=_bad(_frame(2), 0.5, 0))), ValueError, "not normalised"),
    (lambda: ((_obs(), _azim(), _elev(), 100.0), dict(hits=_hits(), vec_north=_frame(1), vec_norm=_bad(_frame(2), np.nan, 0))), ValueError, "not normalised"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_invalid_arguments_raise_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().panorama(*args, **kw)


def test_type_errors_come_before_value_errors(no_library):
    """A wrong type is reported although an earlier argument has a wrong value."""
    with pytest.raises(TypeError, match="max_dist"):
        _terrain().panorama(np.ones((S, 4), np.float32), _azim(), _elev(), None, dist=_dist())
    with pytest.raises(TypeError, match="vec_norm"):
        _terrain().panorama(_obs(), _azim(0), _elev(), -1.0, vec_north=_frame(1), vec_norm="up")


def test_elevations_at_the_float32_limits_pass_the_checks():
    """+-float32(pi/2) are inside; the call then reaches the library (here: an uninitialised Terrain)."""
    t = _terrain()
    t._shape = None
    elev = np.array([-HALF_PI, 0.0, HALF_PI], np.float32)
    with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
        t.panorama(_obs(), _azim(), elev, 100.0, dist=_dist((S, 3, A)))


def test_one_array_for_two_outputs(no_library):
    """Two views of one buffer are refused."""
    raw = np.zeros(S * 3 * 4 * 3, np.float32)
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().panorama(_obs(), _azim(4), _elev(3), 100.0, dist=raw[:S * 12].reshape(S, 3, 4), point=raw.reshape(S, 3, 4, 3))
    raw = np.zeros(S * 2, np.float32)
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().panorama(_obs(), _azim(2), _elev(1), 100.0, dist=raw.reshape(S, 1, 2), hits=raw.view(np.int64))


def test_torch_tensors_must_be_on_the_terrains_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().panorama(_obs(), _azim(), _elev(), 100.0, dist=torch.zeros((S, E, A), dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().panorama(_obs(), _azim(), _elev(), 100.0, point=torch.zeros((S, E, A, 3), dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().panorama(_obs(), _azim(), _elev(), 100.0, hits=torch.zeros(S, dtype=torch.int64))
    with pytest.raises(ValueError, match="device"):
        _terrain().panorama(torch.ones((S, 3), dtype=torch.float32), _azim(), _elev(), 100.0, hits=_hits())
    with pytest.raises(ValueError, match="dtype"):
        _terrain().panorama(_obs(), _azim(), _elev(), 100.0, dist=torch.zeros((S, E, A), dtype=torch.float64))
    with pytest.raises(ValueError, match="dtype"):
        _terrain().panorama(_obs(), _azim(), _elev(), 100.0, hits=torch.zeros(S, dtype=torch.int32))
    with pytest.raises(TypeError, match="azim"):
        _terrain().panorama(_obs(), torch.zeros(A, dtype=torch.float32), _elev(), 100.0, hits=_hits())


def test_uninitialised_terrain(no_library):
    t = _terrain()
    t._shape = None
    for kw in (dict(dist=_dist()), dict(point=_point()), dict(hits=_hits())):
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            t.panorama(_obs(), _azim(), _elev(), 100.0, **kw)


def test_signature():
    params = inspect.signature(Terrain.panorama).parameters
    assert list(params) == ["self", "observers", "azim", "elev", "max_dist", "dist", "point", "hits", "vec_north", "vec_norm"]
    for name in list(params)[1:5]:
        assert params[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and params[name].default is inspect.Parameter.empty
    for name in list(params)[5:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None


def test_outputs_are_keyword_only(no_library):
    with pytest.raises(TypeError):
        _terrain().panorama(_obs(), _azim(), _elev(), 100.0, _dist())


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.Terrain.panorama is Terrain.panorama


def test_horizon_terrain_has_no_panorama():
    """A stored horizon holds one angle per azimuth, not the surface below the skyline."""
    from horayzon_amd.shadow import HorizonTerrain
    assert not hasattr(HorizonTerrain, "panorama")


def test_documented_where_viewshed_is():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "viewshed" in text and "panorama" in text, name
    assert "clause 20" in " ".join(Terrain.panorama.__doc__.split())


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    decl = re.search(r"int hz_terrain_panorama\((.*?)\);", hdr, flags=re.S)
    assert decl, "hz_terrain_panorama is not declared"
    text = re.sub(r"/\*.*?\*/", " ", decl.group(1), flags=re.S)
    params = [" ".join(p.split()) for p in text.split(",")]
    assert params == ["hz_terrain *terrain", "const float *observers", "int num_obs",
                      "const float *azim_sin", "const float *azim_cos", "int azim_num",
                      "const float *elev_sin", "const float *elev_cos", "int elev_num",
                      "const float *vec_north", "const float *vec_norm", "float max_dist",
                      "float *dist", "float *point", "int64_t *hits", "hz_stats *stats"]
    assert "hz_terrain_panorama" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "hz_terrain_panorama")
    assert len(L.hz_terrain_panorama.argtypes) == 16


def test_abi_revision_and_structs_are_unchanged():
    """An added entry point: no struct grows, the revision stays."""
    import ctypes as C
    L = _lib.lib()
    assert L.hz_abi_version() == 6
    opts, stats = C.c_int(0), C.c_int(0)
    assert L.hz_abi_struct_sizes(C.byref(opts), C.byref(stats)) == 0
    assert stats.value == C.sizeof(_lib.hz_stats)


def test_debug_knobs_exist():
    L = _lib.lib()
    for key in (b"panorama_traversal", b"panorama_budget"):
        assert L.hz_debug_set(key, -1) == 0
    assert L.hz_debug_set(b"panorama_traversal", 2) == 1
    assert b"panorama_traversal" in L.hz_last_error()
    assert L.hz_debug_set(b"panorama_traversal", -1) == 0


def test_c_entry_point_checks_its_arguments():
    """The C entry point's own checks, before any device is touched."""
    L = _lib.lib()
    obs, d = _obs(), _dist()
    tab = np.zeros(8, np.float32)
    p = tab.ctypes.data
    assert L.hz_terrain_panorama(None, obs.ctypes.data, S, p, p, A, p, p, E, None, None, 100.0, d.ctypes.data, None, None, None) == 1
    assert b"not initialised" in L.hz_last_error()
