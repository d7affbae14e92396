"""The flat refill of guess_constant (hz_search.h, advance_guess_flat; k_horizon<..., FLAT>): the transitions of the search state
machine as one branch-free pass.  It makes the same transitions on the same state, so horizon, ray count, guard events and guard
cells are IDENTICAL to what hz_debug_set("flat_refill", 0) -- the instantiations with the state machine's if-chain, in the same
library -- gives, bit for bit, and to the CPU oracle."""
import numpy as np
import pytest

from horayzon_amd import synth
from tests import cases

pytestmark = pytest.mark.gpu

IN0, IN1, RING = 37, 29, 16          # inner domain ragged against the 8 x 8 blocks (5 x 4 of them, 3 x 2 tiles), 16-cell ring
KEYS = ("num_rays", "guard_events", "guard_cells")


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


@pytest.fixture
def schedule(hip):
    def set_(**kw):
        hip.horizon.schedule_overrides.clear()
        hip.horizon.schedule_overrides.update(kw)
    yield set_
    hip.horizon.schedule_overrides.clear()


def _dem(spike=False):
    g = cases.rough_terrain(IN0 + 2 * RING, IN1 + 2 * RING, seed=53, relief=1500.0, offset=RING, tilt_frames=not spike)
    if spike:
        # one vertex 200 km above its neighbours, 30 m away: the facets around it stand steeper than the table's last entry
        # (89.98 degrees: 30 m * tan = 86 km), so the UP search of the cells next to it is still blocked at the top index
        # (the cell on the spike itself is masked: it would add DOWN searches that are free at index 0)
        z = g["z"].copy()
        z[RING + 18, RING + 14] += 2.0e5
        xx, yy = np.meshgrid(g["x"], g["y"])
        g["vert_grid"] = synth.pack_vertices(xx, yy, z)
    return g


def _mask():
    m = np.ones((IN0, IN1), np.uint8)
    m[0, 0] = m[7, 8] = m[8, 7] = m[20, 28] = m[36, 13] = m[36, 28] = 0      # corners, a block seam, the ragged rim
    m[18, 14] = 0                                                            # the cell on the spike of _dem(spike=True)
    return m


_REF = {}


def _run(hip, key, flat, kw, **par):
    """One run per (case, switch), shared by the tests and never modified."""
    if (key, flat) not in _REF:
        with flat_refill(flat):
            h, a = hip.horizon.horizon_gridded(**kw, **par)
            st = dict(hip.horizon.last_stats)
        h.setflags(write=False)
        _REF[(key, flat)] = (h, a, st)
    return _REF[(key, flat)]


def _same(hip, key, kw, **par):
    h0, a0, s0 = _run(hip, key, 0, kw, **par)
    h1, a1, s1 = _run(hip, key, 1, kw, **par)
    print(key, {k: (s0[k], s1[k]) for k in KEYS + ("left_cells", "stack_fallbacks")})
    assert not np.isnan(h0).any()
    assert np.array_equal(h0.view(np.uint32), h1.view(np.uint32)) and np.array_equal(a0, a1)
    for k in KEYS:
        assert s0[k] == s1[k], k
    return h0, s0, s1


def _par(azim_num, **kw):
    return dict(dict(dist_search=2.0, azim_num=azim_num, ray_algorithm="guess_constant", elev_ang_low_lim=-60.0,
                     mask=_mask(), hori_fill=-2.5), **kw)


@pytest.mark.parametrize("azim_num", (4, 6, 8, 90, 360))
def test_small_dem_flat_against_state_machine(hip, azim_num):
    """azim_num 6 and 90 are no multiple of 4: the instantiations without output staging."""
    kw = cases.grid_kwargs(_dem())
    h, s0, _ = _same(hip, ("dem", azim_num), kw, **_par(azim_num))
    assert s0["num_cells"] == int(_mask().sum()) and s0["stack_fallbacks"] == 0
    assert np.all(h[_mask() != 1] == np.float32(-2.5))


def test_up_search_reaches_the_top_index(hip):
    kw = cases.grid_kwargs(_dem(spike=True))
    _, s0, _ = _same(hip, "spike", kw, **_par(36))
    assert s0["guard_events"] > 0                      # or the test proves nothing


def test_down_search_reaches_index_zero(hip):
    """elev_ang_low_lim = +5 degrees: wherever the horizon lies lower, the DOWN search is still free at index 0."""
    kw = cases.grid_kwargs(_dem())
    _, s0, _ = _same(hip, "low", kw, **_par(36, elev_ang_low_lim=5.0))
    assert s0["guard_events"] > 0


def test_hand_over_mid_search(hip, schedule):
    """persist_grid=2: 8 waves share the 24 blocks; left_min=0x18: a block ends at 24 unfinished cells and the follow-up (LEFT)
    launch restores their search states mid-search.  Production and follow-up launch both flat, then both with the if-chain --
    and the same again for the DEM whose searches end at the table's top."""
    schedule(persist_grid=2, left_min=0x18)
    for key, spike in (("left", False), ("left_spike", True)):
        kw = cases.grid_kwargs(_dem(spike=spike))
        _, s0, s1 = _same(hip, key, kw, **_par(360))
        assert s0["left_cells"] > 0 and s1["left_cells"] > 0
    # the schedule does not change the result either
    h_plain = _run(hip, ("dem", 360), 0, cases.grid_kwargs(_dem()), **_par(360))[0]
    assert np.array_equal(_REF[("left", 1)][0], h_plain)


def test_counting_instantiation(hip):
    kw = cases.grid_kwargs(_dem())
    res = {}
    for flat in (0, 1):
        with flat_refill(flat):
            h, _ = hip.horizon.horizon_gridded(**kw, **_par(90), count_work=True)
            res[flat] = (h, dict(hip.horizon.last_stats))
    (h0, s0), (h1, s1) = res[0], res[1]
    print({k: (s0[k], s1[k]) for k in KEYS + ("nodes_visited", "tris_tested", "wave_refills")})
    assert np.array_equal(h0.view(np.uint32), h1.view(np.uint32))
    for k in KEYS + ("nodes_visited", "tris_tested"):
        assert s0[k] == s1[k], k
    assert s0["nodes_visited"] > 0 and s0["tris_tested"] > 0
    assert np.array_equal(h0, _run(hip, ("dem", 90), 1, kw, **_par(90))[0])


@pytest.mark.parametrize("case", ("dem", "spike"))
def test_against_the_oracle(hip, orc, case):
    kw = cases.grid_kwargs(_dem(spike=(case == "spike")))
    par = _par(90) if case == "dem" else _par(36)
    h_cpu, a_cpu, so = orc.horizon_gridded(**kw, **par, return_stats=True)
    h, a, st = _run(hip, ("dem", 90) if case == "dem" else "spike", 1, kw, **par)
    assert np.array_equal(a, a_cpu) and np.array_equal(h, h_cpu)
    assert st["num_rays"] == so["rays"] and st["guard_events"] == so["guards"]
