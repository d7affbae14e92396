"""HorizonTerrain.refraction (hz_horizon_terrain_refraction): argument checks, the declaration and the export.  No GPU needed:
every check here fires before anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import HorizonTerrain
from tests.test_horisun_args import SHAPE, _terrain, no_library  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _elev(shape=SHAPE, dtype=np.float32):
    return np.zeros(shape, dtype)


BAD = [
    (lambda: _elev().tolist(), TypeError, "'elevation' has incorrect type"),
    (lambda: _elev(dtype=np.float64), ValueError, "dtype mismatch, expected 'float32'"),
    (lambda: _elev(SHAPE + (1,)), ValueError, "wrong number of dimensions"),
    (lambda: _elev((6, 8)), ValueError, "array 'elevation' has incorrect shape"),
    (lambda: _elev(SHAPE[::-1]), ValueError, "array 'elevation' has incorrect shape"),
    (lambda: _elev(SHAPE[::-1]).T, ValueError, "array 'elevation' is not C-contiguous"),
    (lambda: _elev((SHAPE[0], 2 * SHAPE[1]))[:, ::2], ValueError, "array 'elevation' is not C-contiguous"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD)
def test_refraction_rules_fire_before_the_library(no_library, make, exc, pattern):
    t = _terrain()
    with pytest.raises(exc, match=pattern):
        t.refraction(make())
    assert t.refrac_cor is False


def test_no_range_check_as_in_terrain(monkeypatch):
    """Any float32 values reach the library, None reaches it as a null pointer, and the property follows."""
    seen = []

    class Lib:
        def hz_horizon_terrain_refraction(self, h, elevation, stats):
            seen.append(elevation)
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    t = _terrain()
    assert t.refrac_cor is False
    wild = np.full(SHAPE, -1.0e30, np.float32)
    wild[0, 0] = np.nan
    t.refraction(wild)
    assert seen == [wild.ctypes.data] and t.refrac_cor is True
    t.refraction(None)
    assert seen[1] is None and t.refrac_cor is False


def test_a_failing_call_leaves_refraction_off(monkeypatch):
    class Lib:
        def hz_horizon_terrain_refraction(self, h, elevation, stats):
            return 1

        def hz_last_error(self):
            return b"boom"
    t = _terrain()
    t._refrac = True
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    with pytest.raises(_lib.HorayzonHipError):
        t.refraction(_elev())
    assert t.refrac_cor is False


def test_initialise_switches_refraction_off(monkeypatch):
    from tests.test_horisun_args import _init_args

    class Lib:
        def hz_horizon_terrain_initialise(self, *a):
            return 0

        def hz_horizon_terrain_initialise_planes(self, *a):
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    for planes in (False, True):
        t = _terrain()
        t._refrac = True
        a = _init_args()
        if planes:
            a["hori"] = np.ascontiguousarray(np.moveaxis(a["hori"], 2, 0))
            t.initialise_azim_major(**a)
        else:
            t.initialise(**a)
        assert t.refrac_cor is False


def test_not_initialised(no_library):
    t = _terrain(shape=None)
    for arg in (_elev(), None):
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            t.refraction(arg)


def test_property_is_read_only_and_documented():
    assert isinstance(HorizonTerrain.refrac_cor, property) and HorizonTerrain.refrac_cor.fset is None
    assert list(inspect.signature(HorizonTerrain.refraction).parameters) == ["self", "elevation"]
    for doc in (HorizonTerrain.__doc__, HorizonTerrain.initialise.__doc__, HorizonTerrain.initialise_azim_major.__doc__):
        assert "refraction" in doc and "not covered" not in doc and "No atmospheric refraction" not in doc


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.HorizonTerrain.refraction is HorizonTerrain.refraction


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int hz_horizon_terrain_refraction(hz_horizon_terrain* t, const float* elevation , hz_stats* stats );" in flat
    L = _lib.lib()
    assert "hz_horizon_terrain_refraction" in _lib.SYMBOLS and hasattr(L, "hz_horizon_terrain_refraction")
    assert len(L.hz_horizon_terrain_refraction.argtypes) == 3
    assert L.hz_abi_version() == 6                               # additive: the revision of the existing structs stays


def test_c_entry_point_checks_its_handle():
    L = _lib.lib()
    assert L.hz_horizon_terrain_refraction(None, _elev().ctypes.data, None) == 1
    assert b"not initialised" in L.hz_last_error()
    assert L.hz_horizon_terrain_refraction(None, None, None) == 1
