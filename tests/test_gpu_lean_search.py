"""The lean search state of the flat guess_constant refill (hz_search.h: SearchLean; k_horizon<..., FLAT>): the binary search of
azimuth 0 keeps lim_up / lim_low in the lane's words of the two LDS rows below the fast stack -- rows 2 and 3 of the staging buffer
when the output is staged (azim_num % 4 == 0), the two padding rows otherwise -- and a cell handed over in that phase carries them
in words 7 and 8 of its record.  Nothing the search decides changes, so every case is IDENTICAL, bit for bit, to the same call
under hz_debug_set("flat_refill", 0) (the instantiations with the full Search struct, same library): horizon, sky view factor, ray
count, guard events and the cells handed over.  Against the CPU oracle the horizon, the ray count and the guard events are identical
too; the sky view factor is a float32 reduction on the device and is held to the oracle's at 1e-5, the bound the rest of the suite
holds the fused sky view factor to (one azimuth has no sky view factor: that case compares the rest)."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

KEYS = ("num_rays", "guard_events", "guard_cells", "left_cells")
ACC = 0.25      # hori_acc [degrees]


class flat_refill:
    """hz_debug_set("flat_refill", value) for the block, the default (on) restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"flat_refill", self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"flat_refill", 1))


def _dem(n, seed=61):
    """n x n inner cells of rough terrain in a 12-cell ring, frames tilted as on a curved DEM."""
    return cases.rough_terrain(n + 24, n + 24, seed=seed, relief=1500.0, offset=12, tilt_frames=True)


def _tilt(n):
    rng = np.random.default_rng(7)
    a, b = rng.uniform(-0.3, 0.3, (n, n)), rng.uniform(-0.3, 0.3, (n, n))
    return np.stack([np.sin(b), -np.sin(a) * np.cos(b), np.cos(a) * np.cos(b)], axis=2).astype(np.float32)


def _par(azim_num, **kw):
    return dict(dict(dist_search=2.0, azim_num=azim_num, hori_acc=ACC, ray_algorithm="guess_constant", elev_ang_low_lim=-60.0), **kw)


_ORC = {}


def _oracle(orc, key, kw, par):
    """One oracle run per input, shared by the cases that use it and never modified."""
    if key not in _ORC:
        h, a, so = orc.horizon_gridded(**kw, **par, return_stats=True)
        h.setflags(write=False)
        _ORC[key] = (h, a, so)
    return _ORC[key]


def _check(hip, orc, key, n, par, **sched):
    kw = cases.grid_kwargs(_dem(n))
    tilt = _tilt(n) if par["azim_num"] >= 2 else None
    extra = dict(sched, **({"svf_vec_tilt": tilt} if tilt is not None else {}))
    res = {}
    for flat in (0, 1):
        with flat_refill(flat):
            out = hip.horizon.horizon_gridded(**kw, **par, **extra)
            res[flat] = (out, dict(hip.horizon.last_stats))
    (o0, s0), (o1, s1) = res[0], res[1]
    print(key, {k: (s0[k], s1[k]) for k in KEYS + ("stack_fallbacks",)})
    assert not np.isnan(o1[0]).any()
    assert np.array_equal(o0[0].view(np.uint32), o1[0].view(np.uint32)) and np.array_equal(o0[1], o1[1])
    for k in KEYS:
        assert s0[k] == s1[k], k
    h_cpu, a_cpu, so = _oracle(orc, key, kw, par)
    assert np.array_equal(o1[1], a_cpu) and np.array_equal(o1[0].view(np.uint32), h_cpu.view(np.uint32))
    assert s1["num_rays"] == so["rays"] and s1["guard_events"] == so["guards"]
    if tilt is not None:
        assert np.array_equal(o0[2].view(np.uint32), o1[2].view(np.uint32))
        svf_cpu = orc.sky_view_factor(a_cpu, h_cpu, tilt)
        err = float(np.abs(o1[2] - svf_cpu).max())
        print(key, "svf against the oracle: max abs difference", err)
        assert err <= 1.0e-5
    assert s1["num_cells"] == n * n
    return h_cpu, s1


def test_staging_rows(hip, orc):
    """8 azimuths: the output is staged, the two LDS words are rows 2 and 3 of the staging buffer (row 2 is staged into at azimuths
    2 and 6, after the binary search is over)."""
    _check(hip, orc, ("dem", 8), 24, _par(8))


def test_padding_rows(hip, orc):
    """6 azimuths: no staging, the two LDS words are the padding rows."""
    _check(hip, orc, ("dem", 6), 24, _par(6))


@pytest.mark.parametrize("azim_num", (8, 6))
def test_several_blocks_per_wave_and_hand_over(hip, orc, azim_num):
    """_persist_grid=2: 8 waves share the 9 blocks, so a wave's LDS rows serve one block after the other; _left_min=40: a block ends
    at 40 unfinished cells and the follow-up launch restores them."""
    _, st = _check(hip, orc, ("dem", azim_num), 24, _par(azim_num), _persist_grid=2, _left_min=40)
    assert st["left_cells"] > 0


@pytest.mark.parametrize("low", (20.0, -89.98))
def test_binary_search_ends_at_a_table_end(hip, orc, low):
    """elev_ang_low_lim = +20 degrees: the horizon of most cells lies below the table, every ray of their binary search is free and
    azimuth 0 ends at index 0 (and the DOWN searches of the later azimuths run into index 0: guard events).  -89.98 degrees: the
    widest table, the longest binary search."""
    h_cpu, st = _check(hip, orc, ("low", low), 24, _par(8, elev_ang_low_lim=low))
    if low > 0:
        assert (h_cpu[:, :, 0] <= np.float32(np.deg2rad(low + ACC))).any()      # azimuth 0 ended within hori_acc of the table's low end
        assert st["guard_events"] > 0


def test_hand_over_in_azimuth_0(hip, orc):
    """One azimuth, _left_min=40: every ray belongs to the binary search, so the cells a block hands over are in PH_BIN and their
    records carry the two LDS values in words 7 and 8; the follow-up launch puts them back into its own rows."""
    _, st = _check(hip, orc, ("one", 1), 16, _par(1), _left_min=40)
    assert st["left_cells"] > 0
