"""HorizonTerrain.sun_times on the GPU (clause 14) against the NumPy reference
(tests/suntimes_reference.py), against the device's own shadow codes, and across layouts, position chunks, the refraction
switch, output kinds and the edge cases.

Bars.  A cell is held to the reference unless one of its positions has |g| <= 1e-9 rad (clause 10's margin for the float64
look-up) or one of its transitions has |g_prev - g| < 1e-3 rad; at most 1 % of a case's unmasked cells may be so excluded
(tests/test_suntimes_reference.py: the cases exclude 0 - 0.12 %).  For the others a look-up disagreement E <= 1e-9 rad moves
the interpolation weight of a crossing by at most E / |g_prev - g| <= 1e-6, so sunrise and sunset are within
1e-6 * max(diff(times)) + one float32 spacing of the reference, duration within 2 * intervals * 1e-6 * max(diff(times)) + one
float32 spacing; intervals and the NaN, 0 and fill patterns are exact.  Everything the device is compared with on itself --
layouts, chunks, output kinds, the switch off again -- is compared word for word."""
import ctypes as C

import numpy as np
import pytest

from horayzon_amd.shadow import gridded_azimuths
from tests import suntimes_reference as T

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("sunrise", "sunset", "duration", "intervals")


class debug_set:
    """hz_debug_set(key, value) for the block, the default restored afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, -1))
        return False


def chunk(k):
    return debug_set(b"horisun_chunk", k)


def make(hip, c, planes=False, refrac=None):
    """refrac None: on exactly when the case has a refraction factor."""
    t = hip.shadow.HorizonTerrain()
    hori = np.ascontiguousarray(c["hori"].transpose(2, 0, 1)) if planes else c["hori"]
    (t.initialise_azim_major if planes else t.initialise)(
        gridded_azimuths(c["azim_num"]), hori, c["vert_grid"], c["dem_dim_0"], c["dem_dim_1"], c["offset_0"], c["offset_1"],
        c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], c["mask"], sw_dir_cor_fill=c["fill"],
        ang_max=c["ang_max"])
    if (c["fac"] is not None) if refrac is None else refrac:
        t.refraction(c["elevation"])
    return t


_OBJ = {}


def obj(hip, name, planes=False):
    """The HorizonTerrain of (case, layout): made once per session; the refraction case's refracts."""
    if (name, planes) not in _OBJ:
        _OBJ[(name, planes)] = make(hip, T.case(name)[0], planes)
    return _OBJ[(name, planes)]


def blank(shape, keys=KEYS):
    return {k: np.full(shape, 77, np.int32 if k == "intervals" else np.float32) for k in keys}


def run(t, suns, times, keys=KEYS):
    out = blank(t._shape, keys)
    t.sun_times(suns, times, **out)
    return out


def words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_words(a, b, keys=KEYS):
    return all(a[k].dtype == b[k].dtype and np.array_equal(words(a[k]), words(b[k])) for k in keys)


_RUNS = {}


def result(hip, name, flavour, planes=False):
    """The maps of (case, flavour, layout) at the test chunk: computed once, never written again."""
    key = (name, flavour, planes)
    if key not in _RUNS:
        c, _ = T.case(name)
        with chunk(T.CHUNK_TEST):                                 # S = 13 runs in five launches, the last with one position
            out = run(obj(hip, name, planes), c["suns"], c["times"][flavour])
        for a in out.values():
            a.setflags(write=False)
        _RUNS[key] = out
    return _RUNS[key]


def hold_to_reference(label, c, ref, times, out):
    """The bars of the module docstring; prints every figure before it asserts."""
    mask = c["mask"]
    unmasked, scored = mask == 1, T.scored(c, ref)
    tol_rise, tol_set, tol_dur = T.tolerances(ref, times)
    with np.errstate(all="ignore"):
        err = {k: np.abs(out[k].astype(np.float64) - ref[k].astype(np.float64)) for k in KEYS[:3]}
    lit = scored & (ref["intervals"] > 0)

    def worst(e, tol):
        return float((e[lit] / tol[lit]).max()) if lit.any() else 0.0
    print("%s: %d unmasked, %d excluded, %d scored and lit; worst error / tolerance: sunrise %.3g, sunset %.3g, duration %.3g; "
          "intervals differ in %d scored cells (%d of the excluded)"
          % (label, int(unmasked.sum()), int((unmasked & ~scored).sum()), int(lit.sum()), worst(err["sunrise"], tol_rise),
             worst(err["sunset"], tol_set), worst(err["duration"], tol_dur),
             int((out["intervals"] != ref["intervals"])[scored].sum()),
             int((out["intervals"] != ref["intervals"])[unmasked & ~scored].sum())))
    assert (unmasked & ~scored).sum() <= T.CAP * unmasked.sum()
    # exact: the number of spells and the NaN / 0 pattern of the scored cells, the fill and -1 of the masked ones
    assert np.array_equal(out["intervals"][scored], ref["intervals"][scored])
    for k in KEYS[:3]:
        assert np.array_equal(np.isnan(out[k][scored]), np.isnan(ref[k][scored])), k
        if np.isnan(c["fill"]):
            assert np.isnan(out[k][~unmasked]).all(), k
        else:
            assert (out[k][~unmasked] == F(c["fill"])).all(), k
    assert (out["intervals"][~unmasked] == -1).all()
    never = scored & (ref["intervals"] == 0)
    assert np.isnan(out["sunrise"][never]).all() and np.isnan(out["sunset"][never]).all()
    assert (out["duration"][never] == 0.0).all() and (out["intervals"][never] == 0).all()
    # within the derived tolerance
    assert (err["sunrise"][lit] <= tol_rise[lit]).all()
    assert (err["sunset"][lit] <= tol_set[lit]).all()
    assert (err["duration"][lit] <= tol_dur[lit]).all()


# ---- 1. the four maps against the reference --------------------------------------------------------------------------------

@pytest.mark.parametrize("planes", (False, True))
@pytest.mark.parametrize("flavour", T.FLAVOURS)
@pytest.mark.parametrize("name", T.NAMES)
def test_matches_the_reference(hip, name, flavour, planes):
    c, refs = T.case(name)
    out = result(hip, name, flavour, planes)
    hold_to_reference("%s %s planes=%d" % (name, flavour, planes), c, refs[flavour], c["times"][flavour], out)


# ---- 2. against the device's own shadow codes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("planes", (False, True))
@pytest.mark.parametrize("name", T.NAMES)
def test_intervals_are_the_runs_of_the_devices_shadow_code_zero(hip, name, planes):
    c, _ = T.case(name)
    t = obj(hip, name, planes)
    suns, times = c["suns"], c["times"]["uniform"]
    codes = np.full((suns.shape[0],) + t._shape, 77, np.uint8)
    t.shadow_batch(suns, codes)
    out = result(hip, name, "uniform", planes)
    unmasked = c["mask"] == 1
    assert (codes[:, ~unmasked] == 3).all()
    # no exclusions: g never decides the lit state
    assert np.array_equal(out["intervals"][unmasked], T.runs_of_zero(codes)[unmasked])
    assert np.array_equal((out["sunrise"] == F(times[0]))[unmasked], (codes[0] == 0)[unmasked])
    assert np.array_equal((out["sunset"] == F(times[-1]))[unmasked], (codes[-1] == 0)[unmasked])


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", T.FLAVOURS)
@pytest.mark.parametrize("name", T.NAMES)
def test_both_layouts_give_the_same_words(hip, name, flavour):
    assert same_words(result(hip, name, flavour, False), result(hip, name, flavour, True))


# ---- 4. position chunks ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes", (False, True))
@pytest.mark.parametrize("name", T.MAIN + (T.REFRAC,))
def test_the_position_chunk_changes_no_word(hip, name, planes):
    c, _ = T.case(name)
    t = obj(hip, name, planes)
    suns, times = c["suns"], c["times"]["uneven"]
    at_three = result(hip, name, "uneven", planes)                 # five launches
    with chunk(1):                                                # one position per launch
        assert same_words(run(t, suns, times), at_three)
    assert same_words(run(t, suns, times), at_three)              # the default: one launch, no state array


# ---- 5. refraction ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("planes", (False, True))
def test_refraction_on_and_off_again(hip, planes):
    c, refs = T.case(T.REFRAC)
    suns, times = c["suns"], c["times"]["uniform"]
    t = make(hip, c, planes, refrac=False)
    with chunk(T.CHUNK_TEST):
        plain = run(t, suns, times)
        hold_to_reference("plain planes=%d" % planes, c, T.case_plain_reference(T.REFRAC, "uniform"), times, plain)
        t.refraction(c["elevation"])
        bent = run(t, suns, times)
        hold_to_reference("refracted planes=%d" % planes, c, refs["uniform"], times, bent)
        assert same_words(bent, result(hip, T.REFRAC, "uniform", planes))
        assert not same_words(bent, plain)
        t.refraction(None)
        assert same_words(run(t, suns, times), plain)


# ---- 6. output kinds -------------------------------------------------------------------------------------------------------

def test_torch_and_numpy_outputs_and_every_subset_give_the_same_words(hip):
    import torch
    from horayzon_amd import _lib
    name = "inner_A7_random"
    c, _ = T.case(name)
    t = obj(hip, name)
    suns, times = c["suns"], c["times"]["uneven"]
    want = result(hip, name, "uneven")
    with chunk(T.CHUNK_TEST):
        dev = {k: torch.full(t._shape, 77, dtype=torch.int32 if k == "intervals" else torch.float32, device="cuda:0") for k in KEYS}
        t.sun_times(suns, times, **dev)
        assert same_words({k: v.cpu().numpy() for k, v in dev.items()}, want)
        # positions in HBM
        t.sun_times(torch.from_numpy(suns).to("cuda:0"), times, **dev)
        assert same_words({k: v.cpu().numpy() for k, v in dev.items()}, want)
        # any subset: the 14 proper ones
        for bits in range(1, 15):
            keys = tuple(k for i, k in enumerate(KEYS) if bits >> i & 1)
            assert same_words(run(t, suns, times, keys), want, keys), keys
        # the C entry point with times in HBM, host positions and mixed outputs
        d_times = torch.from_numpy(times).to("cuda:0")
        host = blank(t._shape, ("sunrise", "intervals"))
        d_dur = torch.full(t._shape, 77.0, dtype=torch.float32, device="cuda:0")
        out = _lib.hz_suntimes_out(sunrise=host["sunrise"].ctypes.data, duration=d_dur.data_ptr(),
                                   intervals=host["intervals"].ctypes.data)
        L = _lib.lib()
        _lib.check(L.hz_horizon_terrain_sun_times(t._h, suns.ctypes.data, d_times.data_ptr(), suns.shape[0], C.byref(out), None))
        host["duration"] = d_dur.cpu().numpy()
        assert same_words(host, want, ("sunrise", "duration", "intervals"))
        # times in HBM are checked too
        d_bad = d_times.clone()
        d_bad[5] = d_bad[4]
        assert L.hz_horizon_terrain_sun_times(t._h, suns.ctypes.data, d_bad.data_ptr(), suns.shape[0], C.byref(out), None) == 1
        assert b"strictly increasing" in L.hz_last_error()
    # launches of two positions, each input from its own side: positions in HBM with host times, and the other way round
    with chunk(2):
        mixed = blank(t._shape)
        t.sun_times(torch.from_numpy(suns).to("cuda:0"), times, **mixed)
        assert same_words(mixed, want)
        mixed = blank(t._shape)
        out4 = _lib.hz_suntimes_out(**{k: v.ctypes.data for k, v in mixed.items()})
        _lib.check(L.hz_horizon_terrain_sun_times(t._h, suns.ctypes.data, d_times.data_ptr(), suns.shape[0], C.byref(out4), None))
        assert same_words(mixed, want)


def test_c_entry_point_refuses_bad_arguments(hip):
    from horayzon_amd import _lib
    L = _lib.lib()
    name = "cell_A360_random"
    c, _ = T.case(name)
    t = obj(hip, name)
    suns, times = c["suns"], c["times"]["uniform"]
    a, b = np.zeros(t._shape, np.float32), np.zeros(t._shape, np.int32)
    S = suns.shape[0]

    def call(num=S, tm=times, **kw):
        out = _lib.hz_suntimes_out(**kw)
        return L.hz_horizon_terrain_sun_times(t._h, suns.ctypes.data, tm.ctypes.data, num, C.byref(out), None)
    assert call(num=0, sunrise=a.ctypes.data) == 1 and b"sun_positions" in L.hz_last_error()
    assert call() == 1 and b"no output buffer" in L.hz_last_error()
    assert call(sunrise=a.ctypes.data, sunset=a.ctypes.data) == 1 and b"different arrays" in L.hz_last_error()
    bad = times.copy()
    bad[3] = np.nan
    assert call(tm=bad, intervals=b.ctypes.data) == 1 and b"finite and strictly increasing" in L.hz_last_error()
    out = _lib.hz_suntimes_out(sunrise=a.ctypes.data)
    out.size = 8
    assert L.hz_horizon_terrain_sun_times(t._h, suns.ctypes.data, times.ctypes.data, S, C.byref(out), None) == 1
    assert b"hz_suntimes_out.size" in L.hz_last_error()
    assert call(sunrise=a.ctypes.data, intervals=b.ctypes.data) == 0


# ---- 7. edges --------------------------------------------------------------------------------------------------------------

def test_one_position(hip):
    c, refs = T.case("one_position")
    t = obj(hip, "one_position")
    times = c["times"]["uniform"]
    out = run(t, c["suns"], times)
    codes = np.empty((1,) + t._shape, np.uint8)
    t.shadow_batch(c["suns"], codes)
    lit, unmasked = codes[0] == 0, c["mask"] == 1
    assert lit.any() and (unmasked & ~lit).any()
    assert (out["sunrise"][lit] == F(times[0])).all() and (out["sunset"][lit] == F(times[0])).all()
    assert (out["duration"][lit] == 0.0).all() and (out["intervals"][lit] == 1).all()
    dark = unmasked & ~lit
    assert np.isnan(out["sunrise"][dark]).all() and np.isnan(out["sunset"][dark]).all()
    assert (out["duration"][dark] == 0.0).all() and (out["intervals"][dark] == 0).all()


def test_all_cells_masked(hip):
    c, _ = T.case("all_masked")
    out = run(obj(hip, "all_masked"), c["suns"], c["times"]["uneven"])
    assert all(np.isnan(out[k]).all() for k in KEYS[:3]) and (out["intervals"] == -1).all()


def test_fill_value_and_never_lit_cells(hip):
    c, refs = T.case("fill_minus_one")
    out = result(hip, "fill_minus_one", "uniform")
    masked = c["mask"] != 1
    assert masked.any()
    assert all((out[k][masked] == F(-1.0)).all() for k in KEYS[:3]) and (out["intervals"][masked] == -1).all()
    never = ~masked & (out["intervals"] == 0)
    assert never.any()
    assert np.isnan(out["sunrise"][never]).all() and np.isnan(out["sunset"][never]).all() and (out["duration"][never] == 0.0).all()
    assert not np.isnan(out["duration"][~masked]).any()


def test_scratch_does_not_grow_with_the_track(hip):
    name = "inner_A360_planar"
    c, _ = T.case(name)
    t = obj(hip, name)
    suns, times = c["suns"], c["times"]["uniform"]
    cells = c["mask"].size
    with chunk(T.CHUNK_TEST):
        run(t, suns, times)
        short = t.last_stats["scratch_bytes"]
        twice = run(t, np.concatenate([suns, suns]), np.concatenate([times, times + 24.0]))
        assert t.last_stats["scratch_bytes"] == short
        # the state (44 B per cell), positions and times of one chunk, the staging of four host outputs
        assert short == 44 * cells + T.CHUNK_TEST * (8 + 12) + 4 * 4 * cells
        assert t.last_stats["num_cells"] == cells and t.last_stats["t_kernel_s"] > 0.0
    # the track twice: the spells of both days, the first day's sunrise
    once = result(hip, name, "uniform")
    unmasked = c["mask"] == 1
    assert np.array_equal(twice["intervals"][unmasked], 2 * once["intervals"][unmasked])
    assert np.array_equal(words(twice["sunrise"]), words(once["sunrise"]))
    # one launch: no state array
    run(t, suns, times)
    assert t.last_stats["scratch_bytes"] == suns.shape[0] * (8 + 12) + 4 * 4 * cells
