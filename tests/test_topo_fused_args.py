"""The fused horizon reductions (horizon_gridded(topo=...), topo_param.topo_parameters, hz_topo_out, hz_topo_params):
argument checks, the ctypes mirror of hz_topo_out and the exported symbols.  No GPU needed: every check here fires before
anything reaches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import horayzon_amd
from horayzon_amd import _lib
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def grid():
    g = cases.rough_terrain(24, 28, seed=5, offset=4)
    kw = cases.grid_kwargs(g)
    tilt = np.zeros(kw["vec_norm"].shape, np.float32)
    tilt[..., 2] = 1.0
    return kw, tilt


BAD_TOPO_CALLS = [
    # (extra keywords, message pattern)
    (dict(topo=("svf", "slope")), "unknown name"),
    (dict(topo=("openness", "")), "unknown name"),
    (dict(topo=()), "empty"),
    (dict(topo=[]), "empty"),
    (dict(topo=("svf",)), "topo_vec_tilt"),
    (dict(topo=("vsf", "openness")), "topo_vec_tilt"),
    (dict(topo=("svf",), azim_num=1, tilt=True), "azim_num"),
    (dict(topo=("vsf",), azim_num=1, tilt=True), "azim_num"),
    (dict(topo=("openness",), tilt="short"), "shape of topo_vec_tilt"),
    (dict(topo=("svf", "vsf"), tilt="short"), "shape of topo_vec_tilt"),
    (dict(topo_only=True), "topo_only"),
    (dict(topo_only=True, svf_vec_tilt=True), "topo_only"),
    (dict(topo=("openness",), svf_vec_tilt=True), "svf_vec_tilt"),
    (dict(topo=("openness",), svf_only=True, svf_vec_tilt=True), "svf_only"),
    (dict(topo=("svf",), svf_only=True, tilt=True), "svf_only"),
]


@pytest.mark.parametrize("extra,pattern", BAD_TOPO_CALLS)
def test_horizon_gridded_topo_validation(grid, no_library, extra, pattern):
    kw, tilt = grid
    extra = dict(extra)
    t = extra.pop("tilt", None)
    if t is True:
        extra["topo_vec_tilt"] = tilt
    elif t == "short":
        extra["topo_vec_tilt"] = np.ascontiguousarray(tilt[1:])
    if extra.get("svf_vec_tilt") is True:
        extra["svf_vec_tilt"] = tilt
    extra.setdefault("azim_num", 12)
    with pytest.raises(ValueError, match=pattern):
        horayzon_amd.horizon.horizon_gridded(**kw, dist_search=1.0, **extra)


def test_horizon_gridded_topo_vec_tilt_dtype(grid, no_library):
    kw, tilt = grid
    with pytest.raises(ValueError, match="dtype"):
        horayzon_amd.horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=12, topo=("svf",),
                                             topo_vec_tilt=tilt.astype(np.float64))
    with pytest.raises(TypeError, match="topo_vec_tilt"):
        horayzon_amd.horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=12, topo=("svf",),
                                             topo_vec_tilt=tilt.tolist())


def test_reference_checks_still_come_first(grid, no_library):
    """The reference's own checks keep their order: a bad ray_algorithm is reported before a bad topo name."""
    kw, _ = grid
    with pytest.raises(ValueError, match="ray_algorithm"):
        horayzon_amd.horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=12, ray_algorithm="x", topo=("nope",))


def test_openness_alone_needs_no_tilt_and_one_azimuth_passes_the_checks(grid, monkeypatch):
    """Openness divides by azim_num and reads no tilt: with one azimuth and no topo_vec_tilt the call gets as far as
    the library (here a stub that records the call)."""
    kw, _ = grid
    seen = []

    class Stop(Exception):
        pass

    def stub():
        seen.append(1)
        raise Stop()
    monkeypatch.setattr(_lib, "lib", stub)
    with pytest.raises(Stop):
        horayzon_amd.horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=1, topo=("openness",), topo_only=True)
    assert seen == [1]


BAD_PARAM_CALLS = [
    (lambda a, h, t: dict(azim=a, hori=h, vec_tilt=t, which=()), "empty"),
    (lambda a, h, t: dict(azim=a, hori=h, vec_tilt=t, which=("svf", "sky")), "unknown name"),
    (lambda a, h, t: dict(azim=a, hori=h, which=("svf",)), "vec_tilt"),
    (lambda a, h, t: dict(azim=a, hori=h, which=("openness", "vsf")), "vec_tilt"),
    (lambda a, h, t: dict(azim=a[:-1], hori=h, vec_tilt=t), "shapes"),
    (lambda a, h, t: dict(azim=a[:-1], hori=h, which=("openness",)), "shapes"),
    (lambda a, h, t: dict(azim=a, hori=h, vec_tilt=t[1:]), "shapes"),
    (lambda a, h, t: dict(azim=a, hori=h, vec_tilt=t[..., :2]), "shapes"),
    (lambda a, h, t: dict(azim=a, hori=h.astype(np.float64), vec_tilt=t), "data type"),
    (lambda a, h, t: dict(azim=a, hori=h, vec_tilt=t.astype(np.float64)), "data type"),
    (lambda a, h, t: dict(azim=a.astype(np.float64), hori=h, which=("openness",)), "data type"),
    (lambda a, h, t: dict(azim=a[:1], hori=h[..., :1], vec_tilt=t, which=("vsf",)), "shapes"),
]


@pytest.mark.parametrize("make,pattern", BAD_PARAM_CALLS)
def test_topo_parameters_validation(no_library, make, pattern):
    azim = np.linspace(0.0, 2.0 * np.pi, 8, endpoint=False).astype(np.float32)
    hori = np.zeros((3, 4, 8), np.float32)
    tilt = np.zeros((3, 4, 3), np.float32)
    tilt[..., 2] = 1.0
    with pytest.raises(ValueError, match=pattern):
        horayzon_amd.topo_param.topo_parameters(**make(azim, hori, tilt))


def test_hz_topo_params_argument_errors():
    """The C entry point's own checks (before any device is selected)."""
    L = _lib.lib()
    azim = np.zeros(4, np.float32)
    hori = np.zeros((2, 2, 4), np.float32)
    out = np.zeros((2, 2), np.float32)
    p = lambda a: a.ctypes.data                                          # noqa: E731
    assert L.hz_topo_params(p(azim), p(hori), None, 2, 2, 4, None, None, None, 0) == 1
    assert b"no output" in L.hz_last_error()
    assert L.hz_topo_params(p(azim), p(hori), None, 2, 2, 4, None, p(out), None, 0) == 1      # vsf without vec_tilt
    assert L.hz_topo_params(p(azim), p(hori), None, 2, 2, 4, p(out), None, None, 0) == 1      # svf without vec_tilt
    assert L.hz_topo_params(p(azim), p(hori), p(hori), 2, 2, 1, p(out), None, None, 0) == 1   # svf with one azimuth
    assert b"shapes" in L.hz_last_error()


def _header_struct_fields(name):
    hdr = open(os.path.join(ROOT, "include", "horayzon_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"\*?\s*(\w+)\s*;", body)


def test_topo_out_mirror_matches_header():
    """hz_topo_out: the ctypes mirror has the header's fields in the header's order, the compiled offsets and size."""
    names = _header_struct_fields("hz_topo_out")
    assert names == ["size", "vsf", "openness"]
    assert [f for f, _ in _lib.hz_topo_out._fields_] == names
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to check the struct layout"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "horayzon_hip.h"\n'
                    'int main(void) { printf("%zu", sizeof(hz_topo_out));'
                    + "".join(' printf(" %%zu", offsetof(hz_topo_out, %s));' % n for n in names)
                    + " return 0; }\n")
        exe = os.path.join(d, "layout")
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == C.sizeof(_lib.hz_topo_out)
    assert got[1:] == [getattr(_lib.hz_topo_out, n).offset for n in names]
    t = _lib.hz_topo_out()
    assert t.size == C.sizeof(_lib.hz_topo_out) and t.vsf is None and t.openness is None


def test_new_symbols_exported():
    L = _lib.lib()
    for name in ("hz_horizon_gridded_ex", "hz_horizon_gridded_scene_ex", "hz_topo_params"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert L.hz_horizon_gridded_ex.argtypes[-2] is C.POINTER(_lib.hz_topo_out)
    assert L.hz_horizon_gridded_scene_ex.argtypes[-2] is C.POINTER(_lib.hz_topo_out)
    # the _ex forms take the old argument list plus the hz_topo_out pointer in front of the stats
    assert L.hz_horizon_gridded_ex.argtypes[:-2] == L.hz_horizon_gridded.argtypes[:-1]
    assert L.hz_horizon_gridded_scene_ex.argtypes[:-2] == L.hz_horizon_gridded_scene.argtypes[:-1]
