"""The horizon reductions on 16-bit codes and on device tensors (hz_topo_params_q16; sky_view_factor, visible_sky_fraction,
topographic_openness and topo_parameters of horayzon_amd/topo_param.py): argument checks, the declaration and the export.
No GPU needed: every check here fires before anything reaches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from horayzon_amd import _lib, topo_param

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 7)
A = 12
CELL, PLANES = SHAPE + (A,), (A,) + SHAPE
LAYOUT_SHAPE = {"cell_major": CELL, "azim_major": PLANES}


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


def _args(layout, dtype=np.uint16):
    tilt = np.zeros(SHAPE + (3,), np.float32)
    tilt[..., 2] = 1.0
    return dict(azim=np.linspace(0.0, 6.0, A).astype(np.float32), hori=np.zeros(LAYOUT_SHAPE[layout], dtype), vec_tilt=tilt)


def _call(fn, a, layout):
    if fn == "openness":
        return topo_param.topographic_openness(a["azim"], a["hori"], layout=layout)
    if fn == "svf":
        return topo_param.sky_view_factor(a["azim"], a["hori"], a["vec_tilt"], layout=layout)
    if fn == "vsf":
        return topo_param.visible_sky_fraction(a["azim"], a["hori"], a["vec_tilt"], layout=layout)
    return topo_param.topo_parameters(a["azim"], a["hori"], a["vec_tilt"], layout=layout)


FUNCTIONS = ("svf", "vsf", "openness", "all")
SHAPES_MSG = "Inconsistent/incorrect shapes of input arrays"
DTYPES_MSG = "incorrect data type"


# ---- Python ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUT_SHAPE))
@pytest.mark.parametrize("fn", FUNCTIONS)
def test_python_rules_fire_before_the_library(no_library, fn, layout):
    tilted = fn != "openness"
    good = lambda: _args(layout)                                   # noqa: E731
    # wrong dtypes of the horizon: everything but float32 and uint16 (int16 carries codes in tensors only)
    for bad in (np.int16, np.uint8, np.uint32, np.int32, np.float16, np.float64):
        with pytest.raises(ValueError, match=DTYPES_MSG):
            _call(fn, _args(layout, bad), layout)
    a = good()
    a["azim"] = a["azim"].astype(np.float64)
    with pytest.raises(ValueError, match=DTYPES_MSG):
        _call(fn, a, layout)
    if tilted:
        a = good()
        a["vec_tilt"] = a["vec_tilt"].astype(np.float64)
        with pytest.raises(ValueError, match=DTYPES_MSG):
            _call(fn, a, layout)
    # wrong shapes per layout: the other layout's array, one azimuth short, a tilt of another grid
    a = good()
    a["hori"] = np.zeros(LAYOUT_SHAPE["azim_major" if layout == "cell_major" else "cell_major"], np.uint16)
    with pytest.raises(ValueError, match=SHAPES_MSG):
        _call(fn, a, layout)
    a = good()
    a["azim"] = a["azim"][:-1]
    with pytest.raises(ValueError, match=SHAPES_MSG):
        _call(fn, a, layout)
    if tilted:
        a = good()
        a["vec_tilt"] = a["vec_tilt"][:, :-1]
        with pytest.raises(ValueError, match=SHAPES_MSG):
            _call(fn, a, layout)
        a = good()
        a["vec_tilt"] = np.zeros(SHAPE + (2,), np.float32)
        with pytest.raises(ValueError, match=SHAPES_MSG):
            _call(fn, a, layout)
        # len(azim) < 2 with a tilted output
        one = dict(azim=np.zeros(1, np.float32), vec_tilt=good()["vec_tilt"],
                   hori=np.zeros(SHAPE + (1,) if layout == "cell_major" else (1,) + SHAPE, np.uint16))
        with pytest.raises(ValueError, match=SHAPES_MSG):
            _call(fn, one, layout)
    with pytest.raises(ValueError, match="unknown 'layout'"):
        _call(fn, good(), "planes")


def test_python_planes_of_codes_must_be_contiguous(no_library):
    a = _args("azim_major")
    a["hori"] = np.transpose(np.zeros(CELL, np.uint16), (2, 0, 1))
    for fn in FUNCTIONS:
        with pytest.raises(ValueError, match="not C-contiguous"):
            _call(fn, a, "azim_major")
    a["hori"] = np.zeros((A, SHAPE[0], 2 * SHAPE[1]), np.uint16)[:, :, ::2]
    with pytest.raises(ValueError, match="not C-contiguous"):
        _call("all", a, "azim_major")


def test_python_no_output_requested(no_library):
    a = _args("cell_major")
    with pytest.raises(ValueError, match="'which' is empty"):
        topo_param.topo_parameters(a["azim"], a["hori"], a["vec_tilt"], which=())
    with pytest.raises(ValueError, match="unknown name"):
        topo_param.topo_parameters(a["azim"], a["hori"], a["vec_tilt"], which=("svf", "albedo"))
    with pytest.raises(ValueError, match="need 'vec_tilt'"):
        topo_param.topo_parameters(a["azim"], a["hori"], None, which=("vsf",))


def test_python_tensor_rules(no_library):
    torch = pytest.importorskip("torch")
    for layout in sorted(LAYOUT_SHAPE):
        a = _args(layout)
        for dtype in (torch.int16, torch.float32):                # a host tensor is never moved to the device behind the back
            t = dict(a, hori=torch.zeros(LAYOUT_SHAPE[layout], dtype=dtype))
            with pytest.raises(ValueError, match="not on a GPU"):
                _call("all", t, layout)
        for dtype in (torch.int32, torch.float64, torch.uint8):
            with pytest.raises(ValueError, match=DTYPES_MSG):
                _call("openness", dict(a, hori=torch.zeros(LAYOUT_SHAPE[layout], dtype=dtype)), layout)
        with pytest.raises(ValueError, match=SHAPES_MSG):
            _call("all", dict(a, hori=torch.zeros(LAYOUT_SHAPE[layout], dtype=torch.int16)[:-1]), layout)
    # a NumPy horizon with tensors beside it: nowhere for the result to live
    a = _args("cell_major")
    with pytest.raises(ValueError, match="needs a tensor 'hori'"):
        _call("all", dict(a, vec_tilt=torch.from_numpy(a["vec_tilt"])), "cell_major")


def test_python_reaches_the_q16_entry_point(monkeypatch):
    """Codes go to hz_topo_params_q16 with `planes` after the horizon, whichever function is called; float32 keeps its
    entry points."""
    reached = []

    class Lib:
        def hz_topo_params_q16(self, *a):
            reached.append(("q16", a[2], a[4:7], tuple(p is not None for p in a[7:10]), len(a)))
            return 0

        def __getattr__(self, name):
            def other(*a):
                reached.append((name,))
                return 0
            return other
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    want = {"svf": (True, False, False), "vsf": (False, True, False), "openness": (False, False, True), "all": (True,) * 3}
    for layout, planes in (("cell_major", 0), ("azim_major", 1)):
        for fn in FUNCTIONS:
            out = _call(fn, _args(layout), layout)
            assert reached[-1] == ("q16", planes, SHAPE + (A,), want[fn], 11), (layout, fn)
            for m in (out.values() if isinstance(out, dict) else [out]):
                assert isinstance(m, np.ndarray) and m.dtype == np.float32 and m.shape == SHAPE
    _call("svf", _args("cell_major", np.float32), "cell_major")
    assert reached[-1] == ("hz_sky_view_factor",)
    _call("all", _args("azim_major", np.float32), "azim_major")
    assert reached[-1] == ("hz_topo_params_planes",)
    import horayzon
    assert horayzon.topo_param.topo_parameters is topo_param.topo_parameters


# ---- C ABI -------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    proto = ("int hz_topo_params_q16(const float *azim, const uint16_t *hori_q, int planes, const float *vec_tilt, "
             "int len_0, int len_1, int len_2, float *svf, float *vsf, float *openness, int device);")
    assert proto in flat
    assert "topo_planes_direct" in hdr
    L = _lib.lib()
    assert "hz_topo_params_q16" in _lib.SYMBOLS and hasattr(L, "hz_topo_params_q16")
    assert len(L.hz_topo_params_q16.argtypes) == 11
    assert "hz_topo_params_q16" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_abi_revision_and_struct_sizes_are_unchanged():
    L = _lib.lib()
    assert hasattr(L, "hz_topo_params_q16")
    assert L.hz_abi_version() == 6
    a, b = C.c_int(0), C.c_int(0)
    assert L.hz_abi_struct_sizes(C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (C.sizeof(_lib.hz_opts), C.sizeof(_lib.hz_stats)) == (96, 232)


def _err(L):
    return L.hz_last_error() or b""


def test_c_entry_point_checks_its_arguments():
    """HZ_ERR_ARG (1) and topo_api's messages, before any device is touched (no device is present where this runs)."""
    L = _lib.lib()
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    f = L.hz_topo_params_q16
    for planes in (0, 1):
        assert f(p, p, planes, p, 2, 3, 4, None, None, None, 0) == 1 and b"no output requested" in _err(L)
        assert f(None, p, planes, p, 2, 3, 4, p, p, p, 0) == 1 and b"NULL argument" in _err(L)
        assert f(p, None, planes, p, 2, 3, 4, p, p, p, 0) == 1 and b"NULL argument" in _err(L)
        assert f(p, p, planes, None, 2, 3, 4, p, None, None, 0) == 1 and b"NULL argument" in _err(L)
        assert f(p, p, planes, None, 2, 3, 4, None, p, None, 0) == 1 and b"NULL argument" in _err(L)
        assert f(p, p + 1, planes, p, 2, 3, 4, p, p, p, 0) == 1 and b"not aligned to its element type" in _err(L)
        assert f(p, p + 3, planes, None, 2, 3, 4, None, None, p, 0) == 1 and b"not aligned to its element type" in _err(L)
        for lens in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (-1, 3, 4), (2, 3, 1)):
            assert f(p, p, planes, p, *lens, p, p, p, 0) == 1 and b"Inconsistent/incorrect shapes" in _err(L), lens
        assert f(p, p, planes, None, 2, 3, 0, None, None, p, 0) == 1 and b"Inconsistent/incorrect shapes" in _err(L)
    for planes in (2, -1):
        assert f(p, p, planes, p, 2, 3, 4, p, p, p, 0) == 1 and b"planes must be 0 or 1" in _err(L)


def test_topo_planes_direct_knob_is_accepted():
    L = _lib.lib()
    try:
        for v in (1, 0, -1):
            assert L.hz_debug_set(b"topo_planes_direct", v) == 0
    finally:
        L.hz_debug_set(b"topo_planes_direct", 0)
