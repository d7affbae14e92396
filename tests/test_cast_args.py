"""Terrain.cast (hz_terrain_cast): argument checks, the declaration and the export.  No GPU needed: every check here fires
before anything reaches a device."""
import inspect
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib
from horayzon_amd.shadow import Terrain
from tests.terrain_args import _terrain, no_library  # noqa: F401 -- pytest finds the fixture in this namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5


def _org(n=N):
    return np.ones((n, 3), np.float32)


def _dirs(n=N):
    v = np.zeros((n, 3), np.float32)
    v[:, 2] = 1.0
    return v


def _tgt(n=N):
    return np.full((n, 3), 2.0, np.float32)


def _occ(n=N, dtype=np.uint8):
    return np.zeros(n, dtype)


def _dist(n=N, dtype=np.float32):
    return np.zeros(n, dtype)


def _point(shape=(N, 3), dtype=np.float32):
    return np.zeros(shape, dtype)


def _bad(a, value, at=1):
    a = a.copy()
    a.reshape(-1)[at] = value
    return a


def _many(n):
    """n rows of three float32 that cost no memory: a zero-stride view (C-contiguity is checked after the count)."""
    return np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=(n, 3), strides=(0, 0))


# (positional arguments after the Terrain, keywords, exception class, message pattern)
BAD_CALLS = [
    # types
    (lambda: ((_org().tolist(), _dirs()), dict(max_dist=9.0, dist=_dist())), TypeError, "origins"),
    (lambda: ((_org().astype(np.float64), _dirs()), dict(max_dist=9.0, dist=_dist())), ValueError, "dtype"),
    (lambda: ((_org()[0], _dirs()), dict(max_dist=9.0, dist=_dist())), ValueError, "dimensions"),
    (lambda: ((_org(), _dirs().tolist()), dict(max_dist=9.0, dist=_dist())), TypeError, "directions"),
    (lambda: ((_org(), _dirs().astype(np.float64)), dict(max_dist=9.0, dist=_dist())), ValueError, "dtype"),
    (lambda: ((_org(), _dirs()[0]), dict(max_dist=9.0, dist=_dist())), ValueError, "dimensions"),
    (lambda: ((_org(),), dict(targets=(1, 2, 3), dist=_dist())), TypeError, "targets"),
    (lambda: ((_org(),), dict(targets=_tgt().astype(np.float16), dist=_dist())), ValueError, "dtype"),
    (lambda: ((_org(),), dict(targets=_tgt().reshape(N, 3, 1), dist=_dist())), ValueError, "dimensions"),
    (lambda: ((_org(), _dirs()), dict(max_dist="far", dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_org(), _dirs()), dict(max_dist=True, dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_org(), _dirs()), dict(max_dist=np.ones(1, np.float32), dist=_dist())), TypeError, "max_dist"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, occluded=_occ().tolist())), TypeError, "occluded"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, occluded=_occ(dtype=np.bool_))), ValueError, "dtype"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, occluded=_occ(dtype=np.int32))), ValueError, "dtype"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, occluded=_occ().reshape(N, 1))), ValueError, "dimensions"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_point())), ValueError, "dimensions"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=7)), TypeError, "dist"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, point=_point(dtype=np.float64))), ValueError, "dtype"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, point=_dist())), ValueError, "dimensions"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, point="p")), TypeError, "point"),
    # the mode
    (lambda: ((_org(),), dict(max_dist=9.0, dist=_dist())), ValueError, "exactly one of 'directions' and 'targets'"),
    (lambda: ((_org(),), dict(dist=_dist())), ValueError, "exactly one of 'directions' and 'targets'"),
    (lambda: ((_org(), _dirs()), dict(targets=_tgt(), max_dist=9.0, dist=_dist())), ValueError, "exactly one of 'directions' and 'targets'"),
    (lambda: ((_org(), _dirs()), dict(targets=_tgt(), dist=_dist())), ValueError, "exactly one of 'directions' and 'targets'"),
    (lambda: ((_org(), _dirs()), dict(dist=_dist())), ValueError, "'max_dist' must be given with 'directions'"),
    (lambda: ((_org(), _dirs()), dict(max_dist=None, occluded=_occ())), ValueError, "'max_dist' must be given with 'directions'"),
    (lambda: ((_org(),), dict(targets=_tgt(), max_dist=9.0, dist=_dist())), ValueError, "'max_dist' must be None with 'targets'"),
    (lambda: ((_org(),), dict(targets=_tgt(), max_dist=np.inf, dist=_dist())), ValueError, "'max_dist' must be None with 'targets'"),
    # outputs and order
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0)), ValueError, "at least one"),
    (lambda: ((_org(),), dict(targets=_tgt(), occluded=None, dist=None, point=None)), ValueError, "at least one"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(), order="random")), ValueError, "'order' must be"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(), order="Sorted")), ValueError, "'order' must be"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(), order=1)), ValueError, "'order' must be"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(), order=None)), ValueError, "'order' must be"),
    # shapes
    (lambda: ((np.ones((N, 4), np.float32), _dirs()), dict(max_dist=9.0, dist=_dist())), ValueError, "'origins' has incorrect shape"),
    (lambda: ((np.ones((0, 3), np.float32), np.ones((0, 3), np.float32)), dict(max_dist=9.0, dist=_dist(0))), ValueError, "'origins' has incorrect shape"),
    (lambda: ((_many(2 ** 31 - 63), _dirs()), dict(max_dist=9.0, dist=_dist())), ValueError, r"2\*\*31 - 64"),
    (lambda: ((_org(), _dirs(N + 1)), dict(max_dist=9.0, dist=_dist())), ValueError, "'directions' has incorrect shape"),
    (lambda: ((_org(), np.ones((N, 2), np.float32)), dict(max_dist=9.0, dist=_dist())), ValueError, "'directions' has incorrect shape"),
    (lambda: ((_org(),), dict(targets=_tgt(N - 1), dist=_dist())), ValueError, "'targets' has incorrect shape"),
    (lambda: ((_org(),), dict(targets=np.ones((3, N), np.float32), dist=_dist())), ValueError, "'targets' has incorrect shape"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, occluded=_occ(N + 1))), ValueError, "'occluded' has incorrect shape"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(N - 1))), ValueError, "'dist' has incorrect shape"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, point=_point((N, 4)))), ValueError, "'point' has incorrect shape"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, point=_point((3, N)))), ValueError, "'point' has incorrect shape"),
    (lambda: ((np.ones((3, N), np.float32).T, _dirs()), dict(max_dist=9.0, dist=_dist())), ValueError, "C-contiguous"),
    (lambda: ((_org(), np.ascontiguousarray(_dirs().T).T), dict(max_dist=9.0, dist=_dist())), ValueError, "C-contiguous"),
    (lambda: ((_org(),), dict(targets=_tgt(2 * N)[::2], dist=_dist())), ValueError, "C-contiguous"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, occluded=_occ(2 * N)[::2])), ValueError, "C-contiguous"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, dist=_dist(2 * N)[::2])), ValueError, "C-contiguous"),
    (lambda: ((_org(), _dirs()), dict(max_dist=9.0, point=_point((3, N)).T)), ValueError, "C-contiguous"),
    # contents
    (lambda: ((_org(), _dirs()), dict(max_dist=0.0, dist=_dist())), ValueError, "'max_dist' must be finite"),
    (lambda: ((_org(), _dirs()), dict(max_dist=-5.0, dist=_dist())), ValueError, "'max_dist' must be finite"),
    (lambda: ((_org(), _dirs()), dict(max_dist=np.nan, dist=_dist())), ValueError, "'max_dist' must be finite"),
    (lambda: ((_org(), _dirs()), dict(max_dist=np.inf, dist=_dist())), ValueError, "'max_dist' must be finite"),
    (lambda: ((_org(), _dirs()), dict(max_dist=1e39, dist=_dist())), ValueError, "'max_dist' must be finite"),       # infinite as float32
    (lambda: ((_org(), _dirs()), dict(max_dist=1e-60, dist=_dist())), ValueError, "'max_dist' must be finite"),      # zero as float32
    (lambda: ((_bad(_org(), np.nan), _dirs()), dict(max_dist=9.0, dist=_dist())), ValueError, "'origins' has non-finite"),
    (lambda: ((_bad(_org(), -np.inf),), dict(targets=_tgt(), occluded=_occ())), ValueError, "'origins' has non-finite"),
    (lambda: ((_org(), _bad(_dirs(), np.nan)), dict(max_dist=9.0, dist=_dist())), ValueError, "'directions' has non-finite"),
    (lambda: ((_org(), _bad(_dirs(), np.inf)), dict(max_dist=9.0, dist=_dist())), ValueError, "'directions' has non-finite"),
    (lambda: ((_org(),), dict(targets=_bad(_tgt(), np.nan), dist=_dist())), ValueError, "'targets' has non-finite"),
    (lambda: ((_org(),), dict(targets=_bad(_tgt(), np.inf, 14), point=_point())), ValueError, "'targets' has non-finite"),
    (lambda: ((_org(), _dirs() * np.float32(1.01)), dict(max_dist=9.0, dist=_dist())), ValueError, "not normalised"),
    (lambda: ((_org(), _bad(_dirs(), 0.5, 0)), dict(max_dist=9.0, dist=_dist())), ValueError, "not normalised"),
    (lambda: ((_org(), np.zeros((N, 3), np.float32)), dict(max_dist=9.0, dist=_dist())), ValueError, "not normalised"),
    (lambda: ((_org(), _bad(_dirs(), 1.0 + 2e-5, 14)), dict(max_dist=9.0, dist=_dist())), ValueError, "not normalised"),
]


@pytest.mark.parametrize("make,exc,pattern", BAD_CALLS)
def test_invalid_arguments_raise_before_the_library(no_library, make, exc, pattern):
    args, kw = make()
    with pytest.raises(exc, match=pattern):
        _terrain().cast(*args, **kw)


def test_the_rules_fire_in_order(no_library):
    """Types first, then the mode, the outputs, the order, shapes, contiguity, distinct buffers, contents: each call breaks
    a rule and every later one, and the earliest is reported."""
    t = _terrain()
    with pytest.raises(TypeError, match="max_dist"):                       # a type before any value
        t.cast(np.ones((N, 4), np.float32), _dirs(), targets=_tgt(), max_dist="x")
    with pytest.raises(TypeError, match="point"):
        t.cast(_org(), max_dist=-1.0, point=[1.0], order="no")
    with pytest.raises(ValueError, match="exactly one"):
        t.cast(np.ones((N, 4), np.float32), order="no")
    with pytest.raises(ValueError, match="must be given with 'directions'"):
        t.cast(np.ones((N, 4), np.float32), _dirs(), order="no")
    with pytest.raises(ValueError, match="must be None with 'targets'"):
        t.cast(np.ones((N, 4), np.float32), targets=_tgt(), max_dist=-1.0, order="no")
    with pytest.raises(ValueError, match="at least one"):
        t.cast(np.ones((N, 4), np.float32), _dirs(), max_dist=-1.0, order="no")
    with pytest.raises(ValueError, match="'order' must be"):
        t.cast(np.ones((N, 4), np.float32), _dirs(), max_dist=-1.0, dist=_dist(N + 1), order="no")
    with pytest.raises(ValueError, match="'origins' has incorrect shape"):
        t.cast(np.ones((N, 4), np.float32), _dirs(N + 1), max_dist=-1.0, dist=_dist(N + 1))
    with pytest.raises(ValueError, match="'directions' has incorrect shape"):
        t.cast(_org(), _dirs(N + 1), max_dist=-1.0, dist=_dist(N + 1))
    with pytest.raises(ValueError, match="'occluded' has incorrect shape"):
        t.cast(_org(), _dirs(), max_dist=-1.0, occluded=_occ(N + 1), dist=_dist(N + 1))
    with pytest.raises(ValueError, match="'dist' has incorrect shape"):
        t.cast(_org(), _dirs(), max_dist=-1.0, dist=_dist(N + 1), point=_point((N, 2)))
    with pytest.raises(ValueError, match="'point' has incorrect shape"):
        t.cast(np.ones((3, N), np.float32).T, _dirs(), max_dist=-1.0, point=_point((N, 2)))
    raw = np.zeros(4 * N, np.float32)
    with pytest.raises(ValueError, match="C-contiguous"):
        t.cast(np.ones((3, N), np.float32).T, _dirs(), max_dist=-1.0, dist=raw[:N], point=raw[:3 * N].reshape(N, 3))
    with pytest.raises(ValueError, match="different arrays"):
        t.cast(_org(), _dirs(), max_dist=-1.0, dist=raw[:N], point=raw[:3 * N].reshape(N, 3))
    with pytest.raises(ValueError, match="'max_dist' must be finite"):
        t.cast(_bad(_org(), np.nan), _dirs(), max_dist=-1.0, dist=_dist())
    with pytest.raises(ValueError, match="'origins' has non-finite"):
        t.cast(_bad(_org(), np.nan), _bad(_dirs(), np.nan), max_dist=1.0, dist=_dist())
    with pytest.raises(ValueError, match="'directions' has non-finite"):
        t.cast(_org(), _bad(_dirs() * np.float32(2.0), np.nan), max_dist=1.0, dist=_dist())
    with pytest.raises(ValueError, match="not normalised"):
        t.cast(_org(), _dirs() * np.float32(2.0), max_dist=1.0, dist=_dist())


def test_one_array_for_two_outputs(no_library):
    """Two views of one buffer are refused."""
    raw = np.zeros(4 * N, np.float32)
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().cast(_org(), targets=_tgt(), dist=raw[:N], point=raw[:3 * N].reshape(N, 3))
    with pytest.raises(ValueError, match="different arrays"):
        _terrain().cast(_org(), _dirs(), max_dist=5.0, occluded=raw.view(np.uint8)[:N], dist=raw[:N])


def test_unit_rule_is_the_validation_modules(no_library):
    """|sum d^2 - 1| <= 1e-5 passes (the call then reaches the library: here an uninitialised Terrain), beyond it fails."""
    t = _terrain()
    t._shape = None
    ok = _dirs() * np.float32(1.0 + 4e-6)
    with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
        t.cast(_org(), ok, max_dist=5.0, dist=_dist())
    with pytest.raises(ValueError, match="not normalised"):
        t.cast(_org(), _dirs() * np.float32(1.0 + 6e-6), max_dist=5.0, dist=_dist())


def test_torch_tensors_must_be_on_the_terrains_device(no_library):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device"):
        _terrain().cast(torch.ones((N, 3), dtype=torch.float32), _dirs(), max_dist=5.0, dist=_dist())
    with pytest.raises(ValueError, match="device"):
        _terrain().cast(_org(), torch.ones((N, 3), dtype=torch.float32), max_dist=5.0, dist=_dist())
    with pytest.raises(ValueError, match="device"):
        _terrain().cast(_org(), targets=torch.ones((N, 3), dtype=torch.float32), dist=_dist())
    with pytest.raises(ValueError, match="device"):
        _terrain().cast(_org(), _dirs(), max_dist=5.0, occluded=torch.zeros(N, dtype=torch.uint8))
    with pytest.raises(ValueError, match="device"):
        _terrain().cast(_org(), _dirs(), max_dist=5.0, dist=torch.zeros(N, dtype=torch.float32))
    with pytest.raises(ValueError, match="device"):
        _terrain().cast(_org(), _dirs(), max_dist=5.0, point=torch.zeros((N, 3), dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        _terrain().cast(_org(), _dirs(), max_dist=5.0, occluded=torch.zeros(N, dtype=torch.bool))
    with pytest.raises(ValueError, match="dtype"):
        _terrain().cast(_org(), _dirs(), max_dist=5.0, dist=torch.zeros(N, dtype=torch.float64))


def test_uninitialised_terrain(no_library):
    t = _terrain()
    t._shape = None
    for kw in (dict(occluded=_occ()), dict(dist=_dist()), dict(point=_point()), dict(dist=_dist(), order="sorted")):
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            t.cast(_org(), _dirs(), max_dist=100.0, **kw)
        with pytest.raises(_lib.HorayzonHipError, match="not initialised"):
            t.cast(_org(), targets=_tgt(), **kw)


def test_signature():
    params = inspect.signature(Terrain.cast).parameters
    assert list(params) == ["self", "origins", "directions", "targets", "max_dist", "occluded", "dist", "point", "order"]
    assert params["origins"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and params["origins"].default is inspect.Parameter.empty
    assert params["directions"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and params["directions"].default is None
    for name in list(params)[3:8]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None
    assert params["order"].kind is inspect.Parameter.KEYWORD_ONLY and params["order"].default == "given"


def test_targets_and_outputs_are_keyword_only(no_library):
    with pytest.raises(TypeError):
        _terrain().cast(_org(), None, _tgt(), dist=_dist())


def test_alias_package_has_the_method():
    import horayzon
    assert horayzon.shadow.Terrain.cast is Terrain.cast


def test_horizon_terrain_has_no_cast():
    """A stored horizon holds no scene to trace against."""
    from horayzon_amd.shadow import HorizonTerrain
    assert not hasattr(HorizonTerrain, "cast")


def test_documented_where_panorama_is():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "panorama" in text and ("Terrain.cast" in text or "hz_terrain_cast" in text), name
    doc = " ".join(Terrain.cast.__doc__.split())
    assert "clause 21" in doc and "synchronisation" in doc and "sorted" in doc


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    decl = re.search(r"int hz_terrain_cast\((.*?)\);", hdr, flags=re.S)
    assert decl, "hz_terrain_cast is not declared"
    text = re.sub(r"/\*.*?\*/", " ", decl.group(1), flags=re.S)
    params = [" ".join(p.split()) for p in text.split(",")]
    assert params == ["hz_terrain *terrain", "const float *origins", "const float *directions", "const float *targets",
                      "int num_rays", "float max_dist", "int order", "uint8_t *occluded", "float *dist", "float *point",
                      "hz_stats *stats"]
    assert "hz_terrain_cast" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "hz_terrain_cast")
    assert len(L.hz_terrain_cast.argtypes) == 11


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
    for key in (b"cast_budget", b"cast_fast_cap", b"cast_sort_only"):
        assert L.hz_debug_set(key, -1) == 0


def test_c_entry_point_checks_its_arguments():
    """The C entry point's own checks, before any device is touched."""
    L = _lib.lib()
    org, dirs, d = _org(), _dirs(), _dist()
    assert L.hz_terrain_cast(None, org.ctypes.data, dirs.ctypes.data, None, N, 100.0, 0, None, d.ctypes.data, None, None) == 1
    assert b"not initialised" in L.hz_last_error()
