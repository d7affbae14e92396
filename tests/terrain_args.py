"""What the args modules of Terrain's observer and ray calls share (test_viewshed_args, test_sight_height_args,
test_panorama_args, test_cast_args): a library that must not be reached and a Terrain without a device."""
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import Terrain


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


def _terrain(shape=(6, 7)):
    """A Terrain that looks initialised to the Python checks, without a device behind it."""
    t = Terrain.__new__(Terrain)
    t._h = None
    t._shape = shape
    t.device = 0
    t.last_stats = None
    return t
