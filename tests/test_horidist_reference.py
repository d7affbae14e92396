"""The CPU reference of the horizon distance (tests/horidist_reference.py; DESIGN.md section 4, clause 16) against its own
definition, the oracle's any-hit query and a known answer.  No GPU needed."""
import numpy as np
import pytest

from horayzon_amd import synth
from tests import cases
from tests import horidist_reference as ref

TABLES = ((0.25, -15.0), (0.15, -15.0), (1.0, -30.0), (0.1, -89.98), (10.0, -15.0))


@pytest.mark.parametrize("hori_acc,low", TABLES)
def test_index_definition(orc, hori_acc, low):
    """h = elev_ang[i] gives i, the float32 below it i - 1, anything below the table -1, anything above it the last entry,
    NaN stays NaN -- for every entry of the table."""
    ea = orc.tables(4, hori_acc, low, 1.0)["elev_ang"]
    n = len(ea)
    assert ea.dtype == np.float32 and n >= 2 and (np.diff(ea) > 0).all()
    i = np.arange(n)
    assert np.array_equal(ref.table_index(ea, ea), i)
    assert np.array_equal(ref.table_index(ea, np.nextafter(ea, np.float32(-np.inf))), i - 1)
    below = np.array([np.nextafter(ea[0], np.float32(-np.inf)), ea[0] - 1.0, -np.pi, -np.inf], np.float32)
    assert (ref.table_index(ea, below) == -1).all()
    above = np.array([np.nextafter(ea[-1], np.float32(np.inf)), ea[-1] + 1.0, np.pi, np.inf], np.float32)
    assert (ref.table_index(ea, above) == n - 1).all()
    assert np.isnan(ref.table_index(ea, np.array([np.nan], np.float32))).all()
    # the definition itself, entry by entry: the maximum over the entries that are <= h
    h = np.concatenate([ea, np.nextafter(ea, np.float32(-np.inf)), below, above])
    brute = np.array([np.flatnonzero(ea <= v).max(initial=-1) for v in h])
    assert np.array_equal(ref.table_index(ea, h), brute)


def test_hit_rays_are_occluded_and_within_the_search_distance(orc):
    g = cases.rough_terrain(48, 48, seed=7, offset=6)
    kw = cases.grid_kwargs(g)
    hori, _ = orc.horizon_gridded(**kw, dist_search=2.0, azim_num=24)
    valid, org, dirs, tfar = ref.distance_rays(**kw, hori=hori, dist_search=2.0)
    dist = ref.horizon_distance(**kw, hori=hori, dist_search=2.0)
    hit = ~np.isnan(dist)
    assert valid.all() and hit.any() and not hit.all()
    assert tfar == np.float32(2000.0)
    occ = orc.Scene(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"]).occluded(org[hit], dirs[hit], tfar)
    assert occ.all()
    assert (dist[hit] >= 0.0).all() and (dist[hit] <= tfar).all()


def test_hill_has_a_distance_everywhere(orc):
    g = cases.c2_hill()
    kw = cases.grid_kwargs(g)
    hori, _ = orc.horizon_gridded(**kw, dist_search=10.0, azim_num=36, ray_algorithm="guess_constant")
    dist = ref.horizon_distance(**kw, hori=hori, dist_search=10.0)
    assert dist.shape == hori.shape and dist.dtype == np.float32
    assert not np.isnan(dist).any()


def test_masked_cells_and_nan_horizons_have_no_distance(orc):
    g = cases.rough_terrain(24, 26, seed=4, offset=4)
    kw = cases.grid_kwargs(g)
    hori, _ = orc.horizon_gridded(**kw, dist_search=2.0, azim_num=8)
    full = ref.horizon_distance(**kw, hori=hori, dist_search=2.0)
    mask = (np.random.default_rng(1).random(hori.shape[:2]) < 0.7).astype(np.uint8)
    h2 = hori.copy()
    h2[3:5] = np.nan
    part = ref.horizon_distance(**kw, hori=h2, dist_search=2.0, mask=mask)
    gone = (mask != 1)[:, :, None] | np.isnan(h2)
    assert np.isnan(part[gone]).all()
    assert np.array_equal(ref.words(part[~gone]), ref.words(full[~gone]))


def test_vertical_step_known_answer(orc):
    """A flat plain with a step of height H: the rows north of the step are H higher, so the riser is one grid spacing wide
    and its middle lies D north of the cell.  The distance ray of the facing azimuth (north, azimuth 0) has the elevation
    elev_ang[k] and meets the riser at a horizontal distance within half a spacing of D, i.e. at a distance along the ray
    within dx / (2 cos(elev_ang[k])) < dx of D / cos(elev_ang[k])."""
    n, dx, H, off = 64, 30.0, 200.0, 8
    x = (np.arange(n) * dx).astype(np.float32)
    y = ((n - 1 - np.arange(n)) * dx).astype(np.float32)          # row 0 is the northernmost
    xx, yy = np.meshgrid(x, y)
    r_step = 12                                                      # rows 0 ... r_step are high
    z = np.where(np.arange(n)[:, None] <= r_step, H, 0.0).astype(np.float32) + 0.0 * xx
    vec_norm, vec_north = synth.planar_frames(n - 2 * off, n - 2 * off)
    kw = dict(vert_grid=synth.pack_vertices(xx, yy, z), dem_dim_0=n, dem_dim_1=n, vec_norm=vec_norm, vec_north=vec_north,
              offset_0=off, offset_1=off)
    hori, _ = orc.horizon_gridded(**kw, dist_search=5.0, azim_num=4)
    dist = ref.horizon_distance(**kw, hori=hori, dist_search=5.0)
    ea = orc.tables(4, 0.25, -15.0, 5.0)["elev_ang"]
    for row in (30, 40):                                             # two cells of the plain, in the middle column
        i, jc = row - off, (n // 2) - off
        D = (row - (r_step + 0.5)) * dx
        k = max(int(ref.table_index(ea, hori[i, jc, 0:1])[0]) - 5, 0)
        assert 0.0 < ea[k] < np.arctan(H / (D - dx / 2)) and np.cos(ea[k]) > 0.5
        assert abs(float(dist[i, jc, 0]) - D / np.cos(float(ea[k]))) < dx
