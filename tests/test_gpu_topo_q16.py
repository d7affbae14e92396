"""The horizon reductions on the 16-bit horizon code and straight from an azimuth-major horizon (DESIGN.md section 4
clause 17; k_topo_q16, k_topo_planes and k_topo_wide_strided of horayzon_amd/csrc/hz_topo.hip, hz_topo_params_q16).

Two yardsticks per case, on codes `q`:

(a) bit for bit -- as uint32 words, the NaN pattern included -- the map the existing float32 cell-major entry point
    returns on Q.decode(q): the contract of the clause;
(b) independently of any kernel, tests/topo_reference.py evaluated on Q.decode(q), with the bars and the Holder of
    tests/test_gpu_topo_reference.py: openness bit-identical, the one-lane-per-cell ("wide") form with its capped share
    of one-ulp cells, the tiled form -- the direct planes kernel counts as tiled -- within E_ref + 2.4e-7.

Every case runs over both layouts, the tiled form and "topo_wide" 1, the three single-output functions, topo_parameters
for all three maps and for each pair, NumPy in, and once per case and layout tensors in with tensors out.
Every figure is printed before it is asserted (pytest -s)."""
import contextlib
import itertools

import numpy as np
import pytest

from tests import q16_reference as Q
from tests import topo_reference as R
from tests.test_gpu_planes import knob
from tests.test_gpu_topo_reference import LAST_TILED, TILTS, Holder, _terrain_case, topo_wide

pytestmark = pytest.mark.gpu

ALL = R.NAMES
LAYOUTS = ("cell_major", "azim_major")
CELL_COUNTS = (1, 63, 64, 65, 257)
AZIM_COUNTS = (2, 31, 32, 33, 63, 64, 65, 360)
D_Q16 = Q.STEP / 2 + 2.0 ** -24             # |decode(encode(h)) - h| for h in range


def planes_of(a):
    return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(words(a), words(b))


def to_host(t):
    """A float32 device tensor as NumPy, moved as integers (no float copy touches a NaN payload)."""
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    torch.cuda.synchronize()
    return t.view(torch.int32).cpu().numpy().view(np.float32)


def code_tensor(q):
    """Codes on the GPU: int16 carrying the bits (every torch has it)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(q).view(np.int16)).to("cuda:0")


def _paths(T, azim, hori, tilt, names, layout):
    """(label, {name: map}) of every Python entry point that yields some of `names`."""
    single = {}
    if "svf" in names:
        single["svf"] = T.sky_view_factor(azim, hori, tilt, layout=layout)
    if "vsf" in names:
        single["vsf"] = T.visible_sky_fraction(azim, hori, tilt, layout=layout)
    if "openness" in names:
        single["openness"] = T.topographic_openness(azim, hori, layout=layout)
    yield "single", single
    for k in range(1, len(names) + 1):
        if k == 2 or k == len(names):
            for sub in itertools.combinations(names, k):
                yield "+".join(sub), T.topo_parameters(azim, hori, tilt, which=sub, layout=layout)


def _check(hip, label, azim, q, tilt, names=ALL):
    import torch
    T = hip.topo_param
    assert q.dtype == np.uint16
    dec = Q.decode(q)
    ref = R.topo_reference(azim, dec, tilt, which=names)
    tilted = [n for n in names if n != "openness"]
    per = R.topo_reference(azim, dec, tilt, which=tilted, perturb_ulps=2, seed=1) if tilted else {}
    h = Holder(label, ref, per, steep=bool(tilted) and R.max_slope_deg(tilt) > 70.0)
    by_layout = {"cell_major": q, "azim_major": planes_of(q)}
    miss = []
    for form in ("tiled", "wide"):
        wide = form == "wide" or len(azim) > LAST_TILED
        with topo_wide() if form == "wide" else contextlib.nullcontext():
            base = T.topo_parameters(azim, dec, tilt, which=names)          # (a): the float32 cell-major entry point
            for layout in LAYOUTS:
                where = "%s %s" % (form, layout)
                for path, maps in _paths(T, azim, by_layout[layout], tilt, names, layout):
                    for name, got in maps.items():
                        if not (isinstance(got, np.ndarray) and same_words(got, base[name])):
                            miss.append("%s %s %s %s: not the words of the float32 entry point on decode(q)" % (label, where, path, name))
                        h.hold(where, wide, path, name, got)
                # tensors in, tensors out: the codes, the azimuths and the tilt in HBM
                d_q = code_tensor(by_layout[layout])
                d_az = torch.from_numpy(azim).to("cuda:0")
                d_tilt = torch.from_numpy(tilt).to("cuda:0") if tilted else None
                torch.cuda.synchronize()
                got = T.topo_parameters(d_az, d_q, d_tilt, which=names, layout=layout)
                for name in names:
                    if not same_words(to_host(got[name]), base[name]):
                        miss.append("%s %s tensors %s: not the words of the float32 entry point on decode(q)" % (label, where, name))
    h.done()
    assert not miss, "\n".join(miss)


def _codes(rng, shape, A, **kw):
    return Q.encode(R.hori_uniform(rng, shape, A, **kw))


@pytest.mark.parametrize("ncell", CELL_COUNTS)
def test_cell_counts(hip, ncell):
    """One lane, a short last wave, a full wave, a full wave plus one cell, a workgroup plus one cell; 33 azimuths are a full
    block of the tile and one column of the next, and odd: every second cell's row of codes starts at 2 mod 4 bytes."""
    rng = np.random.default_rng(4000 + ncell)
    shape, A = R.grid_shape(ncell), 33
    _check(hip, "q16 cells=%d A=33" % ncell, R.make_azim(A), _codes(rng, shape, A), R.tilt_slopes(rng, shape, 70.0))


@pytest.mark.parametrize("A", AZIM_COUNTS + (3457,))
def test_azimuth_counts(hip, A):
    """Partial and full blocks either side of 32 and 64, odd counts, and 3457: the first count whose table does not fit the
    LDS, which takes the one-lane-per-cell form by itself in both layouts."""
    rng = np.random.default_rng(5000 + A)
    shape = R.grid_shape(257 if A <= 360 else 130)
    _check(hip, "q16 cells=%d A=%d" % (shape[0] * shape[1], A), R.make_azim(A, start=0.0 if A % 2 else 0.37),
           _codes(rng, shape, A), R.tilt_slopes(rng, shape, 70.0))


def test_the_whole_code_table(hip):
    """All 65536 codes as 1024 cells x 64 azimuths: every decode runs, 0xFFFF, 0 and 65534 included."""
    rng = np.random.default_rng(6)
    q = rng.permutation(np.arange(65536, dtype=np.uint32)).astype(np.uint16).reshape(32, 32, 64)
    assert len(np.unique(q)) == 65536
    _check(hip, "q16 code table 1024x64", R.make_azim(64), q, R.tilt_slopes(rng, (32, 32), 70.0))


def test_nan_codes_do_not_leak(hip):
    """0xFFFF in 2 % of the cells and three whole rows of it: the NaN pattern of every map is the reference's (SVF and VSF
    take the plane's own horizon and stay numbers, openness is NaN) and the cells sharing a wave's tile are unaffected."""
    rng = np.random.default_rng(78)
    shape, A = (40, 50), 45
    q = Q.encode(R.add_nans(rng, R.hori_uniform(rng, shape, A), frac_cells=0.02, rows=(0, 17, 39)))
    assert (q == Q.NAN_CODE).any(axis=2).sum() > 150 and (q[17] == Q.NAN_CODE).all()
    _check(hip, "q16 NaN cells=40x50 A=45", R.make_azim(A), q, R.tilt_slopes(rng, shape, 70.0))


@pytest.mark.parametrize("tilt_class", ("up", "le70", "le89.5", "unnormalised"))
def test_tilt_classes(hip, tilt_class):
    rng = np.random.default_rng(sum(map(ord, tilt_class)) + 5)
    shape, A = (5, 205), 90
    q = _codes(rng, shape, A, frac_half_pi=0.05)
    _check(hip, "q16 tilt=%s A=90" % tilt_class, R.make_azim(A, start=0.37), q, TILTS[tilt_class](rng, shape))


def _abi(L, azim, hori_ptr, planes, tilt, shape, A, dev="cuda:0"):
    """hz_topo_params_q16 through ctypes on a device pointer; the three maps as NumPy."""
    import torch
    from horayzon_amd import _lib
    out = torch.full((3,) + shape, float("nan"), dtype=torch.float32, device=dev)
    d_tilt = torch.from_numpy(tilt).to(dev)
    torch.cuda.synchronize()
    _lib.check(L.hz_topo_params_q16(azim.ctypes.data, hori_ptr, planes, d_tilt.data_ptr(), shape[0], shape[1], A,
                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0))
    return to_host(out)


@pytest.mark.parametrize("form", ("tiled", "wide"))
def test_device_view_at_an_odd_element(hip, form):
    """`hori_q` as a device view that starts at element 1 of an allocation -- 2 mod 4 bytes -- in both layouts, rows of 63
    cells (planes of an odd number of cells, so every second plane starts at 2 mod 4 on its own) and 33 azimuths: the maps
    equal those of the same codes in an aligned buffer, and the float32 entry point's on decode(q)."""
    import torch
    from horayzon_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(91)
    shape, A = (5, 63), 33
    azim, tilt = R.make_azim(A), R.tilt_slopes(rng, shape, 70.0)
    q = _codes(rng, shape, A)
    with topo_wide() if form == "wide" else contextlib.nullcontext():
        base = hip.topo_param.topo_parameters(azim, Q.decode(q), tilt)
        for planes, arr in ((0, q), (1, planes_of(q))):
            buf = torch.zeros(arr.size + 3, dtype=torch.int16, device="cuda:0")
            view = buf[1:arr.size + 1]
            view.copy_(code_tensor(arr).reshape(-1))
            aligned = code_tensor(arr)
            assert view.data_ptr() % 4 == 2 and aligned.data_ptr() % 4 == 0
            odd = _abi(L, azim, view.data_ptr(), planes, tilt, shape, A)
            even = _abi(L, azim, aligned.data_ptr(), planes, tilt, shape, A)
            for i, name in enumerate(ALL):
                assert same_words(odd[i], even[i]), (planes, name)
                assert same_words(odd[i], base[name]), (planes, name)


def test_host_planes_of_codes_in_several_staging_chunks(hip):
    """9 rows of 64 cells: slabs of 2 rows (128 cells) and of 4 rows (257 cells) against the whole array in one chunk."""
    rng = np.random.default_rng(92)
    shape, A = (9, 64), 33
    azim, tilt = R.make_azim(A), R.tilt_slopes(rng, shape, 70.0)
    q = Q.encode(R.add_nans(rng, R.hori_uniform(rng, shape, A), frac_cells=0.02, rows=(4,)))
    T = hip.topo_param
    one = T.topo_parameters(azim, planes_of(q), tilt, layout="azim_major")
    base = T.topo_parameters(azim, Q.decode(q), tilt)
    for form in ("tiled", "wide"):
        for cells in (128, 257):
            with topo_wide() if form == "wide" else contextlib.nullcontext():
                with knob(b"planes_chunk", cells, -1):
                    got = T.topo_parameters(azim, planes_of(q), tilt, layout="azim_major")
                ref = T.topo_parameters(azim, Q.decode(q), tilt) if form == "wide" else base
            for name in ALL:
                assert same_words(got[name], ref[name]), (form, cells, name)
                if form == "tiled":
                    assert same_words(got[name], one[name]), (cells, name)


def _float_planes_both_routes(hip, label, azim, hori, tilt):
    T = hip.topo_param
    planes = planes_of(hori)
    for form in ("tiled", "wide"):
        with topo_wide() if form == "wide" else contextlib.nullcontext():
            default = T.topo_parameters(azim, planes, tilt, layout="azim_major")
            with knob(b"topo_planes_direct", 1, 0):
                direct = T.topo_parameters(azim, planes, tilt, layout="azim_major")
                single = T.sky_view_factor(azim, planes, tilt, layout="azim_major")
                with knob(b"planes_chunk", 100, -1):
                    staged = T.topo_parameters(azim, planes, tilt, layout="azim_major")
        for name in ALL:
            assert same_words(direct[name], default[name]), (label, form, name)
            assert same_words(staged[name], default[name]), (label, form, name, "staged")
        assert same_words(single, default["svf"]), (label, form)


@pytest.mark.parametrize("ncell", CELL_COUNTS)
def test_float_planes_direct_equals_the_default_route_cells(hip, ncell):
    """hz_debug_set("topo_planes_direct", 1): float32 planes through k_topo_planes<., float> give, word for word, the maps
    of the transposing route (which stays the default)."""
    rng = np.random.default_rng(7000 + ncell)
    shape, A = R.grid_shape(ncell), 33
    hori = R.add_nans(rng, R.hori_uniform(rng, shape, A), frac_cells=0.05)
    _float_planes_both_routes(hip, "cells=%d" % ncell, R.make_azim(A), hori, R.tilt_slopes(rng, shape, 70.0))


@pytest.mark.parametrize("A", AZIM_COUNTS + (3457,))
def test_float_planes_direct_equals_the_default_route_azimuths(hip, A):
    rng = np.random.default_rng(8000 + A)
    shape = R.grid_shape(257 if A <= 360 else 130)
    hori = R.add_nans(rng, R.hori_uniform(rng, shape, A), frac_cells=0.05)
    _float_planes_both_routes(hip, "A=%d" % A, R.make_azim(A, start=0.37), hori, R.tilt_slopes(rng, shape, 70.0))


def test_float_tensors_in_tensors_out(hip):
    """float32 `hori` as a device tensor in both layouts, azim as NumPy and the tilt as a tensor: the NumPy call's words."""
    import torch
    T = hip.topo_param
    rng = np.random.default_rng(93)
    shape, A = (5, 65), 33
    azim, tilt = R.make_azim(A), R.tilt_slopes(rng, shape, 70.0)
    hori = R.add_nans(rng, R.hori_uniform(rng, shape, A), frac_cells=0.05)
    base = T.topo_parameters(azim, hori, tilt)
    d_tilt = torch.from_numpy(tilt).to("cuda:0")
    for layout, arr in (("cell_major", hori), ("azim_major", planes_of(hori))):
        d_h = torch.from_numpy(arr.view(np.int32)).to("cuda:0").view(torch.float32)
        torch.cuda.synchronize()
        got = T.topo_parameters(azim, d_h, d_tilt, layout=layout)
        for name in ALL:
            assert same_words(to_host(got[name]), base[name]), (layout, name)
        assert same_words(to_host(T.sky_view_factor(azim, d_h, d_tilt, layout=layout)), base["svf"])
        assert same_words(to_host(T.topographic_openness(azim, d_h, layout=layout)), base["openness"])


def test_maps_from_the_codes_of_a_real_horizon(hip):
    """horizon_gridded(hori_dtype="uint16") on rough terrain with masked cells (hori_fill = -0.25), 36 azimuths: the maps
    reduced from the returned codes are the maps of dequantise(codes), word for word, and lie within the quantisation
    bound (DESIGN.md section 4 clause 17) of the maps the same call reduces from the unquantised horizon with topo=."""
    kw, tilt, par = _terrain_case()
    par = dict(par, azim_num=36)
    H, T = hip.horizon, hip.topo_param
    for layout in LAYOUTS:
        q, azim, fused = H.horizon_gridded(**kw, **par, topo=ALL, topo_vec_tilt=tilt, hori_dtype="uint16", layout=layout)
        assert q.dtype == np.uint16
        dec = H.dequantise(q)
        fill = (dec == Q.decode(Q.encode(np.float32([-0.25])))[0]).all(axis=0 if layout == "azim_major" else 2)
        assert fill.sum() >= 40
        from_codes = T.topo_parameters(azim, q, tilt, layout=layout)
        from_float = T.topo_parameters(azim, dec, tilt, layout=layout)
        A = len(azim)
        sector = A * float(np.float32(azim[1] - azim[0])) / (2.0 * np.pi)
        t = tilt.astype(np.float64)
        bound = {"svf": (2.0 * np.hypot(t[..., 0], t[..., 1]) + np.abs(t[..., 2])) * D_Q16 * sector,
                 "vsf": np.full(tilt.shape[:2], D_Q16 * sector), "openness": np.full(tilt.shape[:2], D_Q16)}
        for name in ALL:
            assert same_words(from_codes[name], from_float[name]), (layout, name)
            diff = np.abs(from_codes[name].astype(np.float64) - fused[name].astype(np.float64))
            ratio = float((diff / bound[name]).max())
            print("TOPOQ16 real horizon %-10s %-8s max |codes - unquantised| %.3g, worst ratio to the bound %.3f"
                  % (layout, name, float(diff.max()), ratio))
            assert ratio <= 1.0, (layout, name, ratio)
