"""The trimmed per-iteration path of the lean traversal loop (hz_common.h: hz_trace<..., LEAN>, what k_horizon's FLAT instantiations
call): the second queue-fill mask is formed from the selected node, the stack pointer is moved once per iteration by the sum of
the two fill masks, and the node step stands in one exec-mask branch and writes its results in place.  None of this changes a
decision, so every case is IDENTICAL between hz_debug_set("flat_refill", 1) and 0 in the same library (0 launches the
instantiations with the plain hz_trace, whose machine code did not move): horizon bit for bit, ray count, guard events, guard
cells and the cells handed over, and the sky view factor word for word.  Against the CPU oracle the horizon, the ray count and
the guard events are identical and the sky view factor, a float32 reduction on the device, lies within 1e-5, the bound the rest of
the suite holds it to."""
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


def _rough(n):
    """n x n inner cells of rough terrain (relief 1500 m) in a 12-cell ring, frames tilted as on a curved DEM."""
    return cases.rough_terrain(n + 24, n + 24, seed=61, relief=1500.0, offset=12, tilt_frames=True)


def _planar(n):
    """The same terrain with the planar frames norm = (0, 0, 1), north = (0, 1, 0): the rotation is the identity, so a ray's
    direction is (cos(elev) sin(azim), cos(elev) cos(azim), sin(elev)) itself."""
    return cases.rough_terrain(n + 24, n + 24, seed=67, relief=1500.0, offset=12, tilt_frames=False)


def _tilt(n):
    rng = np.random.default_rng(7)
    a, b = rng.uniform(-0.3, 0.3, (n, n)), rng.uniform(-0.3, 0.3, (n, n))
    return np.stack([np.sin(b), -np.sin(a) * np.cos(b), np.cos(a) * np.cos(b)], axis=2).astype(np.float32)


def _par(azim_num, **kw):
    return dict(dict(dist_search=2.0, azim_num=azim_num, hori_acc=ACC, ray_algorithm="guess_constant", elev_ang_low_lim=-60.0), **kw)


_ORC = {}


def _oracle(orc, key, kw, par, tilt):
    """One oracle run per input, shared by the cases that use it and never modified."""
    if key not in _ORC:
        h, a, so = orc.horizon_gridded(**kw, **par, return_stats=True)
        svf = orc.sky_view_factor(a, h, tilt)
        for x in (h, a, svf):
            x.setflags(write=False)
        _ORC[key] = (h, a, so, svf)
    return _ORC[key]


def _check(hip, orc, key, dem, n, par, **sched):
    kw = cases.grid_kwargs(dem)
    tilt = _tilt(n)
    res = {}
    for flat in (0, 1):
        with flat_refill(flat):
            out = hip.horizon.horizon_gridded(**kw, **par, svf_vec_tilt=tilt, **sched)
            res[flat] = (out, dict(hip.horizon.last_stats))
    (o0, s0), (o1, s1) = res[0], res[1]
    print(key, sched, {k: (s0[k], s1[k]) for k in KEYS + ("stack_fallbacks", "stack_redo_blocks")})
    assert not np.isnan(o1[0]).any()
    # the two forms, same library
    assert np.array_equal(o0[0].view(np.uint32), o1[0].view(np.uint32)) and np.array_equal(o0[1], o1[1])
    for k in KEYS:
        assert s0[k] == s1[k], k
    assert np.array_equal(o0[2].view(np.uint32), o1[2].view(np.uint32))
    # the oracle
    h_cpu, a_cpu, so, svf_cpu = _oracle(orc, key, kw, par, tilt)
    assert np.array_equal(o1[1], a_cpu) and np.array_equal(o1[0].view(np.uint32), h_cpu.view(np.uint32))
    assert s1["num_rays"] == so["rays"] and s1["guard_events"] == so["guards"]
    err = float(np.abs(o1[2] - svf_cpu).max())
    print(key, "svf against the oracle: max abs difference", err)
    assert err <= 1.0e-5
    assert s1["num_cells"] == n * n
    return s0, s1


@pytest.mark.parametrize("azim_num", (8, 6))
def test_queue_fills(hip, orc, azim_num):
    """24 x 24 cells, 9 blocks: both queue places fill in one iteration (the stack pointer moves by two rows), a lane pops its
    sentinel, blocks hand over at the default threshold.  8 azimuths: the staged instantiation; 6: the unstaged one."""
    _check(hip, orc, ("rough", azim_num), _rough(24), 24, _par(azim_num))


@pytest.mark.parametrize("azim_num", (8, 6))
def test_several_blocks_per_wave_with_a_hand_over(hip, orc, azim_num):
    """_persist_grid=2: 8 waves share the 9 blocks; _left_min=40: a block ends at 40 unfinished cells and the follow-up launch (the
    LEFT instantiation, the same loop) finishes them."""
    _, st = _check(hip, orc, ("rough", azim_num), _rough(24), 24, _par(azim_num), _persist_grid=2, _left_min=40)
    assert st["left_cells"] > 0


# Fast-stack entries (the `level_stack` schedule option, negative).  The 24 x 24 case needs 14 entries (measured with this library,
# both forms: no overflow from 14 on).  13, the count closest to that which still overflows, has one block out of entries: it is
# computed again from the redo list.  4, the smallest count the library takes, has every block out of entries -- every deep ray runs
# into the clamp of `sa` -- and the launch is repeated with the level stack.
@pytest.mark.parametrize("entries", (4, 13))
def test_stack_clamp_and_overflow(hip, orc, entries):
    """A wrong `sa` (the one update per iteration, the clamp of the node step that now writes in place) shows here: as a store
    outside the lane's entries, a missed overflow, or a block that is not computed again."""
    s0, s1 = _check(hip, orc, ("rough", 8), _rough(24), 24, _par(8), _level_stack=-entries)
    for st in (s0, s1):
        assert st["stack_fallbacks"] > 0 or st["stack_redo_blocks"] > 0


@pytest.mark.parametrize("low", (-60.0, -89.98))
def test_reciprocals_of_tiny_direction_components(hip, orc, low):
    """Planar frames, 16 x 16 cells, 4 azimuths: the rays of azimuths 0 and 2 have dx = +-0 (or the float32 sine of pi, 1e-7), those
    of azimuths 1 and 3 |dy| = cos(elev) * |float32 cosine of pi / 2| (4e-8): the reciprocals of the ray set-up at their largest,
    and the slabs a ray never leaves.  elev_ang_low_lim = -89.98 degrees: the table reaches +-89.98 degrees, dz comes near 1 and
    dx, dy shrink by another 3e-4.  The refill's reciprocal as v_rcp_f32 + clamp was measured with these cases and not kept, so
    what the case guards now is hz_safe_rcp at its extremes (+-1e30 for +-0, 2.5e7 for 4e-8) under both forms of the loop."""
    _check(hip, orc, ("planar", low), _planar(16), 16, _par(4, elev_ang_low_lim=low))
