"""The compaction threshold of the horizon kernel's traversal loop (hz_n_leave, hz_common.h): rule 1 scales it with the lanes that
entered hz_trace with a ray, rule 0 is the absolute threshold.  Which lanes are refilled when is schedule only (DESIGN.md section
4): horizon, sky view factor, ray count, guard events and guard cells under hz_debug_set("regroup_rule", 1) are IDENTICAL, bit for
bit, to what rule 0 gives in the same library and process -- for blocks of every population, with and without the hand-over to the
follow-up launch, for both stack disciplines and all three search algorithms -- and one case is held to the CPU oracle, so that
"equal to each other" cannot mean "equally wrong"."""
import numpy as np
import pytest

from horayzon_amd import synth
from tests import cases

pytestmark = pytest.mark.gpu

N, RING = 72, 16                     # 72 x 72 DEM, 40 x 40 inner domain: 5 x 5 blocks of 8 x 8 cells
KEYS = ("num_rays", "guard_events", "guard_cells")


class regroup_rule:
    """hz_debug_set("regroup_rule", value) for the block, the default restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"regroup_rule", self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"regroup_rule", -1))


_DEM = {}


def _dem(n=N):
    """(grid keywords, vec_tilt) of the n x n fractal tile; n = 69 gives a 37 x 37 inner domain whose rim blocks hold 40, 25 cells."""
    if n not in _DEM:
        g = synth.fractal_tile(n=n, offset=RING)
        tilt, _ = synth.tilt_from_planar_dem(g["x"], g["y"], g["z"], RING)
        _DEM[n] = (cases.grid_kwargs(g), tilt)
    return _DEM[n]


def _mask_ragged(n=N):
    """Every block of the 40 x 40 domain starts with another population, 8 ... 63 cells: block (bi, bj) keeps its first
    8 + (11 * (5 bi + bj)) % 56 cells in row-major order."""
    in_ = n - 2 * RING
    m = np.zeros((in_, in_), np.uint8)
    for bi in range((in_ + 7) // 8):
        for bj in range((in_ + 7) // 8):
            keep = 8 + (11 * (5 * bi + bj)) % 56
            blk = np.zeros(64, np.uint8)
            blk[:keep] = 1
            sub = m[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8]
            sub[...] = blk.reshape(8, 8)[:sub.shape[0], :sub.shape[1]]
    return m


def _mask_checker(n=N):
    """Checkerboard plus random cells: blocks start at populations 1 ... 63 (one block keeps a single cell, one loses a single one)."""
    in_ = n - 2 * RING
    rng = np.random.default_rng(7)
    ii, jj = np.meshgrid(np.arange(in_), np.arange(in_), indexing="ij")
    m = (((ii + jj) & 1) ^ (rng.random((in_, in_)) < 0.3)).astype(np.uint8)
    m[0:8, 0:8] = 0; m[3, 5] = 1              # population 1
    m[8:16, 8:16] = 1; m[9, 9] = 0            # population 63
    return m


def _mask_one_block(n=N):
    """One full block, everything else masked: its hand-over is the follow-up launch's only group."""
    in_ = n - 2 * RING
    m = np.zeros((in_, in_), np.uint8)
    m[8:16, 8:16] = 1
    return m


def _par(azim_num, **kw):
    return dict(dict(dist_search=1.0, azim_num=azim_num, ray_algorithm="guess_constant", elev_ang_low_lim=-60.0, hori_fill=-2.5), **kw)


_REF = {}


def _run(hip, key, rule, n=N, svf=False, **par):
    """One run per (case, rule), shared by the tests and never modified."""
    if (key, rule) not in _REF:
        kw, tilt = _dem(n)
        with regroup_rule(rule):
            out = hip.horizon.horizon_gridded(**kw, **par, **({"svf_vec_tilt": tilt} if svf else {}))
            st = dict(hip.horizon.last_stats)
        for a in out:
            a.setflags(write=False)
        _REF[(key, rule)] = (out, st)
    return _REF[(key, rule)]


def _same(hip, key, **kw):
    out0, s0 = _run(hip, key, 0, **kw)
    out1, s1 = _run(hip, key, 1, **kw)
    print(key, {k: (s0[k], s1[k]) for k in KEYS + ("left_cells", "left_again", "stack_fallbacks", "stack_redo_blocks")})
    assert len(out0) == len(out1)
    for a0, a1 in zip(out0, out1):
        assert a0.dtype == a1.dtype and a0.shape == a1.shape and a0.tobytes() == a1.tobytes()
    assert not np.isnan(out0[0]).any()
    for k in KEYS:
        assert s0[k] == s1[k], k
    assert s0["num_rays"] > 0
    return out0, s0, s1


@pytest.mark.parametrize("azim_num", (360, 12, 6))
def test_full_blocks_and_svf(hip, azim_num):
    """(6 azimuths: no multiple of 4 -- the instantiations that store without staging)"""
    out, s0, _ = _same(hip, ("full", azim_num), svf=True, **_par(azim_num))
    assert len(out) == 3 and s0["num_cells"] == (N - 2 * RING) ** 2


@pytest.mark.parametrize("azim_num", (360, 12, 6))
def test_ragged_populations(hip, azim_num):
    m = _mask_ragged()
    pops = sorted({int(m[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8].sum()) for bi in range(5) for bj in range(5)})
    assert pops[0] == 8 and pops[-1] == 63 and len(pops) == 25
    out, s0, _ = _same(hip, ("ragged", azim_num), svf=True, **_par(azim_num, mask=m))
    assert s0["num_cells"] == int(m.sum()) and np.all(out[0][m != 1] == np.float32(-2.5))


def test_ragged_rim_of_the_domain(hip):
    """37 x 37 cells: the rim blocks start with 40 (8 x 5) and 25 (5 x 5) cells."""
    _, s0, _ = _same(hip, "rim", n=69, svf=True, **_par(360))
    assert s0["num_cells"] == 37 * 37


def test_checkerboard_populations(hip):
    m = _mask_checker()
    pops = {int(m[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8].sum()) for bi in range(5) for bj in range(5)}
    assert 1 in pops and 63 in pops
    _, s0, _ = _same(hip, "checker", svf=True, **_par(360, mask=m))
    assert s0["num_cells"] == int(m.sum())


def test_no_hand_over(hip):
    """every block runs from 64 cells to 0 through the loop"""
    _, s0, s1 = _same(hip, "noleft", **_par(360), _left_min=-1)
    assert s0["left_cells"] == 0 and s1["left_cells"] == 0


@pytest.mark.parametrize("left_min", (0x24, 0x10))
def test_hand_over_and_follow_up(hip, left_min):
    """the follow-up launch runs its groups down to one record"""
    _, s0, s1 = _same(hip, ("left", left_min), **_par(360), _left_min=left_min)
    assert s0["left_cells"] > 0 and s1["left_cells"] > 0
    full = _run(hip, "noleft", 0, **_par(360), _left_min=-1)[0][0]
    assert np.array_equal(_REF[(("left", left_min), 1)][0][0], full)      # the schedule does not change the result either


def test_last_group_below_the_follow_up_threshold(hip):
    """One block hands over at most 16 cells: the follow-up launch's only group starts below its threshold of 24 lanes."""
    m = _mask_one_block()
    _, s0, s1 = _same(hip, "onegroup", **_par(360, mask=m), _left_min=0x10)
    for s in (s0, s1):
        assert 0 < s["left_cells"] < 24


@pytest.mark.parametrize("persist_grid", (-1, 5))
def test_block_loop(hip, persist_grid):
    """one tile per workgroup, and 5 workgroups that pull the 25 blocks (and the follow-up's groups) from the queues"""
    _, s0, s1 = _same(hip, ("persist", persist_grid), **_par(360), _left_min=0x24, _persist_grid=persist_grid)
    assert s0["left_cells"] > 0 and s1["left_cells"] > 0


def test_level_stack_redo(hip):
    """a fast stack of 4 entries overflows: the blocks are computed again with one entry per tree level, under the rule too"""
    _, s0, s1 = _same(hip, "redo", **_par(36), _level_stack=-4)
    for s in (s0, s1):
        assert s["stack_redo_blocks"] + s["stack_fallbacks"] > 0


@pytest.mark.parametrize("alg", ("binary_search", "discrete_sampling"))
def test_other_algorithms(hip, alg):
    _same(hip, alg, **_par(36, ray_algorithm=alg, mask=_mask_ragged()))


def test_against_the_oracle(hip, orc):
    m = _mask_ragged()
    par = _par(12, mask=m)
    kw, _ = _dem()
    h_cpu, a_cpu, so = orc.horizon_gridded(**kw, **par, return_stats=True)
    for rule in (0, 1):
        (h, a, _svf), st = _run(hip, ("ragged", 12), rule, svf=True, **par)
        assert np.array_equal(a, a_cpu) and np.array_equal(h, h_cpu)
        assert st["num_rays"] == so["rays"] and st["guard_events"] == so["guards"]


def test_counting_instantiation_verifies_the_certificates(hip):
    """count_work with verify_near=1: every shortened ray is traced again over its full length; violations 0 under both rules, and
    the tallies that are functions of the rays alone agree."""
    kw, _ = _dem()
    res = {}
    for rule in (0, 1):
        with regroup_rule(rule):
            h, _ = hip.horizon.horizon_gridded(**kw, **_par(36), count_work=True, _verify_near=1)
            res[rule] = (h, dict(hip.horizon.last_stats))
    (h0, s0), (h1, s1) = res[0], res[1]
    print({k: (s0[k], s1[k]) for k in KEYS + ("nodes_visited", "tris_tested", "wave_refills", "near_verified", "near_violations")})
    assert h0.tobytes() == h1.tobytes()
    # (node visits and triangle tests are NOT compared: an any-hit ray stops at the first blocking leaf it tests, and how many
    #  nodes it has visited by then depends on the wave's votes between node and leaf steps, i.e. on the schedule)
    for k in KEYS + ("rays_shortened", "near_verified"):
        assert s0[k] == s1[k], k
    assert s0["nodes_visited"] > 0 and s1["nodes_visited"] > 0
    assert s0["near_verified"] > 0                      # or the test proves nothing
    assert s0["near_violations"] == 0 and s1["near_violations"] == 0
