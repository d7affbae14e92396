"""Leaf lending in the horizon kernel's leaf step (hz_common.h, hz_trace<..., LEND>): a lane without a leaf tests the second
queued leaf of its DPP partner (lane ^ 1, the neighbouring cell of the 8 x 8 block) with the partner's ray.  The hits are
any-hit and the leaf that blocks a ray is the one the plain schedule finds, so horizon, ray count and guard count stay
IDENTICAL to the CPU oracle; only the work counters of the counting instantiation move.  hz_debug_set("leaf_lend", 0) selects
the instantiation without lending: the reference of case (e)."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

PAR_A = dict(dist_search=2.0, azim_num=36, ray_algorithm="guess_constant", elev_ang_low_lim=-60.0)
PAR_D = dict(dist_search=2.0, azim_num=360, ray_algorithm="guess_constant", elev_ang_low_lim=-60.0)


class leaf_lend:
    """hz_debug_set("leaf_lend", value) for the block, the default (on) restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"leaf_lend", self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"leaf_lend", 1))


@pytest.fixture
def schedule(hip):
    def set_(**kw):
        hip.horizon.schedule_overrides.clear()
        hip.horizon.schedule_overrides.update(kw)
    yield set_
    hip.horizon.schedule_overrides.clear()


def _case_a():
    """Inner domain 21 x 13 on a rugged DEM: odd sizes, so the rim waves have lane pairs with one lane outside the domain."""
    return cases.rough_terrain(21 + 12, 13 + 12, seed=41, relief=1500.0, offset=6, tilt_frames=True)


def _case_d():
    """40 x 44 cells: full and ragged 8 x 8 blocks, several blocks per wave under persist_grid=5.  (Seed 47: the blocks hand 599
    cells over at left_min=0x18, so the follow-up launch's last group has 23 records -- an odd count, one lane pair split.  The
    count is a function of the kernel's schedule: should a later change of the traversal move it to an even number, pick the
    next seed that gives an odd one; seeds 43 - 46 and 48 give 600.)"""
    return cases.rough_terrain(40 + 16, 44 + 16, seed=47, relief=1500.0, offset=8, tilt_frames=True)


_REF = {}


def _oracle(orc, key, kw, **par):
    """One oracle run per case, shared by the tests and never modified."""
    if key not in _REF:
        h, a, so = orc.horizon_gridded(**kw, **par, return_stats=True)
        h.setflags(write=False)
        _REF[key] = (h, a, so)
    return _REF[key]


def _check(hip, orc, key, kw, gpu_extra=None, **par):
    h_cpu, a_cpu, so = _oracle(orc, key, kw, **par)
    h_gpu, a_gpu = hip.horizon.horizon_gridded(**kw, **par, **(gpu_extra or {}))
    st = dict(hip.horizon.last_stats)
    assert np.array_equal(a_gpu, a_cpu)
    assert not np.isnan(h_gpu).any()
    assert np.array_equal(h_gpu, h_cpu)
    assert st["num_rays"] == so["rays"]
    assert st["guard_events"] == so["guards"]
    return h_gpu, st


def test_a_odd_domain(hip, orc):
    kw = cases.grid_kwargs(_case_a())
    _, st = _check(hip, orc, "a", kw, **PAR_A)
    assert st["num_cells"] == 21 * 13 and st["stack_fallbacks"] == 0


def test_b_checkerboard_mask(hip, orc):
    """Every lane pair (columns j, j ^ 1 of one row) has exactly one masked lane."""
    kw = cases.grid_kwargs(_case_a())
    ii, jj = np.meshgrid(np.arange(21), np.arange(13), indexing="ij")
    mask = ((ii + jj) & 1).astype(np.uint8)
    h, st = _check(hip, orc, "b", kw, mask=mask, hori_fill=-2.5, **PAR_A)
    assert st["num_cells"] == int(mask.sum())
    assert np.all(h[mask != 1] == np.float32(-2.5))


def test_c_outer_tin(hip, orc):
    """Lent leaves include single-triangle records (fourth vertex NaN)."""
    g = _case_a()
    vs, nvs, ts, nts = cases.outer_tin(g, margin=400.0, zval=1800.0)
    kw = cases.grid_kwargs(g)
    par = dict(PAR_A, dist_search=6.0, elev_ang_low_lim=-30.0)
    h1, _ = _check(hip, orc, "c", kw, vert_simp=vs, num_vert_simp=nvs, tri_ind_simp=ts, num_tri_simp=nts, **par)
    h0, _ = hip.horizon.horizon_gridded(**kw, **par)
    assert (h1 > h0).any()                                     # the ring is seen: its triangles were tested


def test_d_hand_over_and_follow_up_launch(hip, orc, schedule):
    """persist_grid=5: several blocks per wave; left_min=0x18: a block ends at 24 unfinished cells and the follow-up (LEFT) launch
    finishes them in groups of 64 sorted records, the last group a partial one -- both launches with lending."""
    schedule(persist_grid=5, left_min=0x18)
    kw = cases.grid_kwargs(_case_d())
    _, st = _check(hip, orc, "d", kw, **PAR_D)
    print("left_cells", st["left_cells"], "left_again", st["left_again"], "fallbacks", st["stack_fallbacks"])
    assert st["num_cells"] == 40 * 44
    assert st["left_cells"] > 0 and (st["left_cells"] % 64) % 2 == 1      # the last group: an odd number of records


@pytest.mark.parametrize("case", ("a", "d"))
def test_e_lending_on_against_off(hip, case):
    """The two instantiations of the counting kernel on the same input: same horizon and ray count, fewer wave leaf steps with
    lending (which proves that leaves were lent)."""
    kw = cases.grid_kwargs(_case_a() if case == "a" else _case_d())
    par = PAR_A if case == "a" else PAR_D
    res = {}
    for lend in (0, 1):
        with leaf_lend(lend):
            h, _ = hip.horizon.horizon_gridded(**kw, **par, count_work=True)
            res[lend] = (h, dict(hip.horizon.last_stats))
    (h0, s0), (h1, s1) = res[0], res[1]
    print(case, "wave_leaf_iters", s0["wave_leaf_iters"], "->", s1["wave_leaf_iters"],
          "wave_node_iters", s0["wave_node_iters"], "->", s1["wave_node_iters"],
          "tris_tested", s0["tris_tested"], "->", s1["tris_tested"])
    assert np.array_equal(h0, h1)
    assert s0["num_rays"] == s1["num_rays"] and s0["guard_events"] == s1["guard_events"]
    assert s1["wave_leaf_iters"] < s0["wave_leaf_iters"]
    # and the production instantiations agree with both
    for lend in (0, 1):
        with leaf_lend(lend):
            h, _ = hip.horizon.horizon_gridded(**kw, **par)
            assert np.array_equal(h, h0) and hip.horizon.last_stats["num_rays"] == s0["num_rays"]


def test_f_forced_small_fast_stack(hip, orc):
    """A fast stack of 4 entries (sentinel + 3): blocks overflow and are computed again by the level-stack kernel, which has no
    lending."""
    kw = cases.grid_kwargs(_case_a())
    _, st = _check(hip, orc, "a", kw, gpu_extra=dict(_level_stack=-4), **PAR_A)
    assert st["stack_fallbacks"] >= 1
