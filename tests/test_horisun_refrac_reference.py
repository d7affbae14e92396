"""The NumPy reference of HorizonTerrain with refraction (tests/horisun_refrac_reference.py, DESIGN.md section 4 clause 13):
its float32 set-up held bit for bit to the CPU oracle's Terrain(refrac_cor=True), the GPU file's cases held to the exclusion
cap from the reference alone, and the effect of the refraction pinned, so that a GPU run with the refraction silently off
cannot pass."""
import numpy as np
import pytest

from horayzon_amd import synth
from tests import horisun_reference as R
from tests import horisun_refrac_reference as RR
from tests.test_horisun_reference import one_cell, sun

F = np.float32


def against_the_oracle(orc, vert_grid, d0, d1, off0, off1, vec_tilt, vec_norm, enl, elev, mask, suns, ang_max, fill=-3.0):
    """setup_refrac and the code and value that follow from it when no terrain shades, against oracle.Terrain(refrac_cor=True)
    over the DEM `vert_grid`, at every unmasked (position, cell) where the oracle's ray does not hit (shadow != 2).
    Returns (pairs compared, unmasked pairs, differing words)."""
    n0, n1 = mask.shape
    verts = vert_grid[:3 * d0 * d1].reshape(d0, d1, 3)
    vert = np.ascontiguousarray(verts[off0:off0 + n0, off1:off1 + n1])
    fac = RR.refrac_factor(elev)
    dpm = R.dot_prod_min(ang_max)
    t = orc.Terrain()
    t.initialise(vert_grid, d0, d1, off0, off1, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=fill, ang_max=ang_max,
                 refrac_cor=True)
    compared = differing = 0
    for p in suns:
        o_sh, o_sw = np.empty(mask.shape, np.uint8), np.empty(mask.shape, np.float32)
        t.shadow(p, o_sh)
        t.sw_dir_cor(p, o_sw)
        _, dot_ns, dot_ts = RR.setup_refrac(p, vert, vec_norm, vec_tilt, fac)
        with np.errstate(all="ignore"):
            code = np.where(dot_ts > F(0.0), 0, 1).astype(np.uint8)
            val = np.where(dot_ts > dpm, (dot_ts / np.maximum(dot_ns, dpm)) * enl, F(0.0))
        assert val.dtype == np.float32
        at = (mask == 1) & (o_sh != 2)
        assert (o_sh[mask != 1] == 3).all() and (o_sw[mask != 1] == F(fill)).all()
        compared += int(at.sum())
        differing += int((code[at] != o_sh[at]).sum()) + int((val[at].view(np.uint32) != o_sw[at].view(np.uint32)).sum())
    return compared, int((mask == 1).sum()) * len(suns), differing


def test_setup_restates_the_oracle_on_a_flat_dem(orc):
    """A flat DEM of 40 x 40 vertices: tilts up to 80 degrees, elevations from 0 to 4500 m, 14 suns from -0.45 degrees true
    elevation (refraction lifts them above the plane) to the zenith (NaN direction: self-shaded), ang_max 89 and 85."""
    n, off = 40, 3
    rng = np.random.default_rng(31)
    x = (np.arange(n) * 25.0).astype(np.float32)
    y = ((n - 1 - np.arange(n)) * 25.0).astype(np.float32)
    xx, yy = np.meshgrid(x, y)
    vert_grid = synth.pack_vertices(xx, yy, np.full((n, n), 250.0, np.float32))
    n0 = n1 = n - 2 * off
    vec_norm, _ = synth.planar_frames(n0, n1)
    ang = np.deg2rad(80.0) * rng.random((n0, n1))
    dirn = rng.uniform(0.0, 2.0 * np.pi, (n0, n1))
    vec_tilt = np.stack([np.sin(ang) * np.cos(dirn), np.sin(ang) * np.sin(dirn), np.cos(ang)], axis=2).astype(np.float32)
    enl = rng.uniform(1.0, 2.0, (n0, n1)).astype(np.float32)
    mask = (rng.random((n0, n1)) > 0.1).astype(np.uint8)
    elev = rng.uniform(0.0, 4500.0, (n0, n1)).astype(np.float32)
    az = rng.uniform(0.0, 2.0 * np.pi, 14)
    el = np.deg2rad(np.array([-0.45, -0.3, -0.1, 0.0, 0.05, 0.3, 0.9, 1.1, 3.0, 10.0, 30.0, 60.0, 89.0, 90.0]))
    suns = (1.5e11 * np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)).astype(np.float32)
    for ang_max in (89.0, 85.0):
        compared, unmasked, differing = against_the_oracle(orc, vert_grid, n, n, off, off, vec_tilt, vec_norm, enl, elev, mask,
                                                           suns, ang_max)
        print("flat, ang_max %g: %d of %d unmasked pairs compared, %d differing words" % (ang_max, compared, unmasked, differing))
        assert differing == 0
        assert 2 * compared >= unmasked


@pytest.mark.parametrize("name", RR.NAMES)
def test_setup_restates_the_oracle_with_the_cases_arrays(orc, name):
    """The case's frames, tilts, elevations, mask and suns over a flat DEM of the case's size (no relief: few rays hit)."""
    c, _ = RR.case(name)
    d0, d1 = c["dem_dim_0"], c["dem_dim_1"]
    if min(d0, d1) < 2:
        return                                                   # a DEM without a triangle: the oracle builds no scene
    x = (np.arange(d1) * 30.0).astype(np.float32)
    y = ((d0 - 1 - np.arange(d0)) * 30.0).astype(np.float32)
    xx, yy = np.meshgrid(x, y)
    vert_grid = synth.pack_vertices(xx, yy, np.full((d0, d1), 250.0, np.float32))
    compared, unmasked, differing = against_the_oracle(
        orc, vert_grid, d0, d1, c["offset_0"], c["offset_1"], c["vec_tilt"], c["vec_norm"], c["surf_enl_fac"], c["elevation"],
        c["mask"], c["suns"], c["ang_max"])
    print("%s: %d of %d unmasked pairs compared, %d differing words" % (name, compared, unmasked, differing))
    assert differing == 0
    assert 2 * compared >= unmasked


@pytest.mark.parametrize("name", RR.NAMES)
def test_gpu_cases_respect_the_exclusion_cap(name):
    c, ref = RR.case(name)
    share = R.inside_margin_share(c, ref)
    print("%s: share of unmasked pairs inside the margin %.3g" % (name, share))
    assert share <= R.CAP
    assert (ref["code"][:, c["mask"] != 1] == 3).all()


@pytest.mark.parametrize("name", RR.LOW_SUN)
def test_refraction_decides_the_low_sun_cases(name):
    c, ref = RR.case(name)
    plain = R.reference(c)
    on = c["mask"] == 1
    changed = int((ref["code"][:, on] != plain["code"][:, on]).sum())
    pairs = int(on.sum()) * c["suns"].shape[0]
    print("%s: refraction changes %d of %d shadow codes (%.2f %%)" % (name, changed, pairs, 100.0 * changed / pairs))
    assert 100 * changed >= pairs
    assert all((ref["code"][:, on] == k).any() for k in (0, 1, 2))


def test_cases_cover_the_issue():
    assert set(RR.LOW_SUN) == {"low_A360_planar", "coarse_low_A360_planar"} and len(RR.COARSE) == 2
    for name in RR.NAMES:
        c, _ = RR.case(name)
        assert c["elevation"].shape == c["mask"].shape and c["elevation"].dtype == np.float32
        assert c["elevation"].min() >= -400.0 and c["elevation"].max() <= 5000.0
        assert c["suns"].shape[0] in (1, 6, 7) and (c["suns"].shape[0] == 1 or c["suns"].shape[0] > RR.CHUNK_TEST)
    for name in RR.LOW_SUN:
        c, _ = RR.case(name)
        assert c["hori"].min() >= F(-0.02) and c["hori"].max() <= F(0.05)
        el = np.rad2deg(np.arcsin(c["suns"][:, 2].astype(np.float64) / np.linalg.norm(c["suns"].astype(np.float64), axis=1)))
        assert el.min() > -1.21 and el.max() < 3.01


def _codes(c, p, elevation):
    fac = RR.refrac_factor(np.full((1, 1), elevation, np.float32))
    plain = R.lookup(p[None, :], c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"],
                     c["mask"], c["fill"])
    bent = RR.lookup_refrac(p[None, :], c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"],
                            c["mask"], c["fill"], 89.0, fac)
    return int(plain["code"][0, 0, 0]), int(bent["code"][0, 0, 0])


def test_known_answers_on_a_flat_cell():
    # 0.1 degrees true elevation under a horizon of 0.005 rad (0.29 degrees): terrain-shaded; refraction lifts the sun by
    # about 0.55 degrees at sea level: lit
    assert _codes(one_cell([0.005] * 8), sun(123.0, np.deg2rad(0.1)), 0.0) == (2, 0)
    # 0.2 degrees below the cell's plane, nothing on the horizon: self-shaded; lifted above the plane: lit
    assert _codes(one_cell([-1.0] * 8), sun(200.0, np.deg2rad(-0.2)), 0.0) == (1, 0)


def test_refraction_at_sea_level_is_saemundssons():
    """The correction [degree] at sea level against the formula in float64: 1.02 / tan(h + 10.3 / (h + 5.11)) arc minutes,
    times the pressure / temperature factor of the standard atmosphere at 0 m (283.15 K, 101 kPa)."""
    fac = RR.refrac_factor(np.zeros((), np.float32))
    assert abs(float(fac) - 283.0 / (273.0 + 10.0)) < 1e-6
    for h in (-1.0, 0.0, 0.5, 3.0, 45.0, 90.0):
        want = (1.02 / np.tan(np.deg2rad(h + 10.3 / (h + 5.11))) + 0.0019279) * float(fac) / 60.0
        got = float(RR.atmos_refrac(np.float32(h), fac))
        assert abs(got - want) <= 2e-6 * max(abs(want), 1e-3), (h, got, want)
    # the clamp to [-1, 90]
    assert RR.atmos_refrac(np.float32(-5.0), fac) == RR.atmos_refrac(np.float32(-1.0), fac)
