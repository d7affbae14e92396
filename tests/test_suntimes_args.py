"""HorizonTerrain.sun_times (hz_horizon_terrain_sun_times): every argument rule in its order, the declaration and the export.
No GPU needed: every check here fires before anything reaches a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import HorizonTerrain, Terrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
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


def _times(n=S):
    return np.arange(n, dtype=np.float64)


def _out(shape=SHAPE, dtype=np.float32):
    return np.zeros(shape, dtype)


def _bad_times(i, v):
    t = _times()
    t[i] = v
    return t


# (positional arguments, keyword arguments, exception class, message pattern): the type checks in the order of the
# arguments, then every rule of the table in its order
RULES = [
    (lambda: ((_sun().tolist(), _times()), dict(sunrise=_out())), TypeError, "'sun_positions' has incorrect type"),
    (lambda: ((_sun().astype(np.float64), _times()), dict(sunrise=_out())), ValueError, "dtype mismatch, expected 'float32'"),
    (lambda: ((np.ones(3, np.float32), _times()), dict(sunrise=_out())), ValueError, "wrong number of dimensions"),
    (lambda: ((_sun(), _times().tolist()), dict(sunrise=_out())), TypeError, "'times' has incorrect type"),
    (lambda: ((_sun(), _times().astype(np.float32)), dict(sunrise=_out())), ValueError, "dtype mismatch, expected 'float64'"),
    (lambda: ((_sun(), _times().reshape(S, 1)), dict(sunrise=_out())), ValueError, "wrong number of dimensions"),
    (lambda: ((_sun(), _times()), dict(sunrise=_out().tolist())), TypeError, "'sunrise' has incorrect type"),
    (lambda: ((_sun(), _times()), dict(sunset=_out(dtype=np.float64))), ValueError, "dtype mismatch, expected 'float32'"),
    (lambda: ((_sun(), _times()), dict(duration=_out((2,) + SHAPE))), ValueError, "wrong number of dimensions"),
    (lambda: ((_sun(), _times()), dict(intervals=_out())), ValueError, "dtype mismatch, expected 'int32'"),
    (lambda: ((_sun(), _times()), dict(intervals=_out(dtype=np.int64))), ValueError, "dtype mismatch, expected 'int32'"),
    (lambda: ((_sun(), _times()), dict()), ValueError, "at least one of 'sunrise', 'sunset', 'duration' and 'intervals'"),
    (lambda: ((np.ones((S, 4), np.float32), _times()), dict(sunrise=_out())), ValueError, "'sun_positions' has incorrect shape"),
    (lambda: ((np.ones((0, 3), np.float32), _times(0)), dict(sunrise=_out())), ValueError, "'sun_positions' has incorrect shape"),
    (lambda: ((_sun(), _times(S - 1)), dict(sunrise=_out())), ValueError, "'times' has incorrect shape"),
    (lambda: ((_sun(), _times()), dict(sunrise=_out((6, 8)))), ValueError, "'sunrise' has incorrect shape"),
    (lambda: ((_sun(), _times()), dict(sunrise=_out(), intervals=_out((7, 6), np.int32))), ValueError,
     "'intervals' has incorrect shape"),
    (lambda: ((_sun(), _times()), dict(duration=_out(SHAPE[::-1]).T)), ValueError, "C-contiguous"),
    (lambda: ((np.ones((S, 6), np.float32)[:, ::2], _times()), dict(duration=_out())), ValueError, "C-contiguous"),
    (lambda: ((_sun(), np.arange(2 * S, dtype=np.float64)[::2]), dict(duration=_out())), ValueError, "C-contiguous"),
    (lambda: ((_sun(), _bad_times(2, np.nan)), dict(sunrise=_out())), ValueError, "finite and strictly increasing"),
    (lambda: ((_sun(), _bad_times(4, np.inf)), dict(sunrise=_out())), ValueError, "finite and strictly increasing"),
    (lambda: ((_sun(), _bad_times(3, 2.0)), dict(sunrise=_out())), ValueError, "finite and strictly increasing"),
    (lambda: ((_sun(), _times()[::-1].copy()), dict(sunrise=_out())), ValueError, "finite and strictly increasing"),
]


@pytest.mark.parametrize("make,exc,pattern", RULES)
def test_rules_fire_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().sun_times(*args, **kw)


def test_one_array_for_two_outputs(no_library):
    out = _out()
    with pytest.raises(ValueError, match="must be different arrays"):
        _terrain().sun_times(_sun(), _times(), sunrise=out, duration=out)
    both = np.zeros(SHAPE, np.int32)
    with pytest.raises(ValueError, match="must be different arrays"):
        _terrain().sun_times(_sun(), _times(), sunset=both.view(np.float32), intervals=both)


def test_rules_fire_in_the_tables_order(no_library):
    """Two bad arguments: the earlier rule's message."""
    t = _terrain()
    with pytest.raises(ValueError, match="'sun_positions' has incorrect shape"):
        t.sun_times(np.ones((S, 2), np.float32), _times(S - 1), sunrise=_out())
    with pytest.raises(ValueError, match="'times' has incorrect shape"):
        t.sun_times(_sun(), _times(S + 1), sunrise=_out((6, 8)))
    with pytest.raises(ValueError, match="'sunset' has incorrect shape"):
        t.sun_times(_sun(), _times(), sunset=_out((6, 8)), duration=_out(SHAPE[::-1]).T)
    out = _out(SHAPE[::-1]).T
    with pytest.raises(ValueError, match="C-contiguous"):
        t.sun_times(_sun(), _times(), sunrise=out, sunset=out)
    out = _out()
    with pytest.raises(ValueError, match="must be different arrays"):
        t.sun_times(_sun(), _bad_times(1, np.nan), sunrise=out, sunset=out)


def test_not_initialised(no_library):
    with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
        _terrain(shape=None).sun_times(_sun(), _times(), sunrise=_out())


def test_torch_outputs_must_be_on_the_objects_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().sun_times(_sun(), _times(), sunrise=torch.zeros(SHAPE, dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        _terrain().sun_times(_sun(), _times(), intervals=torch.zeros(SHAPE, dtype=torch.float32))
    with pytest.raises(ValueError, match="dimensions"):
        _terrain().sun_times(_sun(), _times(), duration=torch.zeros((2,) + SHAPE, dtype=torch.float32))


def test_valid_arguments_reach_the_library(monkeypatch):
    """One position and any subset of outputs pass every rule; the struct carries exactly the buffers given."""
    seen = []

    class Lib:
        def hz_horizon_terrain_sun_times(self, h, suns, times, num, out, stats):
            o = out._obj
            seen.append((num, o.size, o.sunrise, o.sunset, o.duration, o.intervals))
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    t = _terrain()
    dur, n = _out(), _out(dtype=np.int32)
    t.sun_times(_sun(1), _times(1), duration=dur, intervals=n)
    assert seen == [(1, C.sizeof(_lib.hz_suntimes_out), None, None, dur.ctypes.data, n.ctypes.data)]
    assert t.last_stats is not None


def test_signature_and_docstring():
    p = inspect.signature(HorizonTerrain.sun_times).parameters
    assert list(p) == ["self", "sun_positions", "times", "sunrise", "sunset", "duration", "intervals"]
    for name in ("sunrise", "sunset", "duration", "intervals"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None
    assert not hasattr(Terrain, "sun_times")                      # the ray path has no clearance to interpolate
    assert "Terrain" in HorizonTerrain.sun_times.__doc__ and "ray" in HorizonTerrain.sun_times.__doc__


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("typedef struct hz_suntimes_out { int32_t size; float* sunrise; float* sunset; float* duration; "
            "int32_t* intervals; } hz_suntimes_out;") in flat
    assert ("int hz_horizon_terrain_sun_times(hz_horizon_terrain* t, const float* sun_positions, const double* times, "
            "int num_sun, const hz_suntimes_out* out, hz_stats* stats);") in flat
    L = _lib.lib()
    assert "hz_horizon_terrain_sun_times" in _lib.SYMBOLS and hasattr(L, "hz_horizon_terrain_sun_times")
    assert len(L.hz_horizon_terrain_sun_times.argtypes) == 6
    assert [f[0] for f in _lib.hz_suntimes_out._fields_] == ["size", "sunrise", "sunset", "duration", "intervals"]
    assert _lib.hz_suntimes_out().size == C.sizeof(_lib.hz_suntimes_out) == 40
    assert L.hz_abi_version() == 6                               # additive: the revision of the existing structs stays
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hz_horizon_terrain_sun_times" in integration and "hz_suntimes_out" in integration


def test_c_entry_point_checks_its_arguments():
    """The C entry point's own checks, before any device is touched."""
    L = _lib.lib()
    sun, times = _sun(), _times()
    out = _lib.hz_suntimes_out(sunrise=_out().ctypes.data)
    assert L.hz_horizon_terrain_sun_times(None, sun.ctypes.data, times.ctypes.data, S, C.byref(out), None) == 1
    assert b"not initialised" in L.hz_last_error()
