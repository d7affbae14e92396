"""The NumPy reference of HorizonTerrain (tests/horisun_reference.py, DESIGN.md section 4 clause 10) pinned by hand-placed
suns and hand-computed horizons, and the GPU file's cases held to the exclusion cap from the reference alone."""
import numpy as np
import pytest

from tests import horisun_reference as R

D = 1.5e11


def one_cell(hori, tilt=(0.0, 0.0, 1.0)):
    """A single cell at the origin under the planar frame: norm = up = z, north = y, so east = north x norm = x."""
    f = lambda v: np.array(v, np.float32).reshape(1, 1, -1)
    return dict(hori=f(hori), vert=f((0.0, 0.0, 0.0)), vec_tilt=f(tilt), vec_norm=f((0.0, 0.0, 1.0)),
                vec_north=f((0.0, 1.0, 0.0)), surf_enl_fac=np.ones((1, 1), np.float32), mask=np.ones((1, 1), np.uint8),
                fill=np.nan)


def sun(az_deg, el_rad):
    """Azimuth clockwise from north, elevation above the horizontal, at the sun's distance."""
    a = np.deg2rad(az_deg)
    return np.array([D * np.cos(el_rad) * np.sin(a), D * np.cos(el_rad) * np.cos(a), D * np.sin(el_rad)], np.float32)


def run(c, suns):
    return R.lookup(np.array(suns, np.float32), c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"],
                    c["surf_enl_fac"], c["mask"], c["fill"])


def test_constant_horizon_lit_iff_the_sun_is_above_it():
    h0 = 0.3
    c = one_cell([h0] * 8)
    azs = (0.0, 17.0, 90.0, 133.0, 180.0, 271.0, 359.5)
    out = run(c, [sun(a, h0 + 0.01) for a in azs] + [sun(a, h0 - 0.01) for a in azs])
    assert (out["code"][:len(azs)] == 0).all() and (out["code"][len(azs):] == 2).all()
    assert (out["val"][:len(azs)] > 0).all() and (out["val"][len(azs):] == 0).all()
    assert np.allclose(out["margin"], 0.01, atol=1e-6)
    # flat cell: sw_dir_cor = sin(elevation) / max(sin(elevation), dot_prod_min) = 1
    assert np.allclose(out["val"][:len(azs)], 1.0, atol=1e-6)


@pytest.mark.parametrize("az,k0,k1,t,h", [
    (0.0, 0, 1, 0.0, 0.1),
    (45.0, 0, 1, 0.5, 0.15),                         # (0.1 + 0.2) / 2
    (90.0, 1, 2, 0.0, 0.2),
    (359.0, 3, 0, 359.0 / 90.0 - 3.0, 0.7 - 0.6 * (359.0 / 90.0 - 3.0)),      # the wrap: 0.106667
])
def test_four_azimuths_interpolation_and_wrap(az, k0, k1, t, h):
    c = one_cell([0.1, 0.2, 0.4, 0.7])               # the horizon towards north, east, south, west
    s, _, _ = R.setup(sun(az, 0.5), c["vert"], c["vec_norm"], c["vec_tilt"])
    got_h, alpha, got_k0, got_k1, got_t = (v[0, 0] for v in R.horizon_at(s, c["vec_norm"], c["vec_north"], c["hori"]))
    if t == 0.0 and az > 0.0:                        # float32 sun: the azimuth may fall a hair short of the table entry
        assert (got_k0, got_k1) in ((k0, k1), (k0 - 1, k0)) and min(got_t, 1.0 - got_t) < 1e-6
    else:
        assert (got_k0, got_k1) == (k0, k1) and abs(got_t - t) < 1e-6
    assert abs(got_h - h) < 1e-6 and abs(alpha - 0.5) < 1e-6
    out = run(c, [sun(az, h + 0.01), sun(az, h - 0.01)])
    assert out["code"][:, 0, 0].tolist() == [0, 2]


def test_one_azimuth():
    c = one_cell([0.25])
    for az in (0.0, 100.0, 200.0, 359.9):
        s, _, _ = R.setup(sun(az, 0.5), c["vert"], c["vec_norm"], c["vec_tilt"])
        h, _, k0, k1, _ = (v[0, 0] for v in R.horizon_at(s, c["vec_norm"], c["vec_north"], c["hori"]))
        assert (k0, k1) == (0, 0) and abs(h - 0.25) < 1e-15
    out = run(c, [sun(77.0, 0.26), sun(77.0, 0.24)])
    assert out["code"][:, 0, 0].tolist() == [0, 2]


def test_sun_at_the_zenith():
    c = one_cell([0.1, 0.2, 0.4, 0.7])
    s, dot_ns, dot_ts = R.setup(np.array([0.0, 0.0, D], np.float32), c["vert"], c["vec_norm"], c["vec_tilt"])
    assert s[0, 0].tolist() == [0.0, 0.0, 1.0] and dot_ns[0, 0] == 1.0 and dot_ts[0, 0] == 1.0
    h, alpha, k0, k1, t = (v[0, 0] for v in R.horizon_at(s, c["vec_norm"], c["vec_north"], c["hori"]))
    assert (k0, k1, t) == (0, 1, 0.0) and h == np.float64(np.float32(0.1)) and alpha == np.pi / 2     # atan2(0, 0) = 0
    out = run(c, [[0.0, 0.0, D]])
    assert out["code"][0, 0, 0] == 0 and out["val"][0, 0, 0] == 1.0


def test_nan_horizon_counts_as_lit():
    c = one_cell([np.nan, 0.9, 0.9, 0.9])
    out = run(c, [sun(10.0, 0.3), sun(100.0, 0.3)])          # the first look-up touches the NaN entry, the second does not
    assert out["code"][:, 0, 0].tolist() == [0, 2]
    assert out["val"][0, 0, 0] > 0 and out["val"][1, 0, 0] == 0
    assert np.isinf(out["margin"][0, 0, 0]) and out["margin"][1, 0, 0] > 0.5


def test_self_shading_ang_max_and_mask():
    c = one_cell([-1.0] * 4, tilt=(np.sin(1.0), 0.0, np.cos(1.0)))      # tilted 1 rad towards east
    out = run(c, [sun(270.0, 0.2), sun(270.0, 1.0 + 0.005), sun(90.0, 0.2)])
    # tilt . s = sin(elevation - 1) for a west sun.  0.2 rad up: behind the tilted surface (1); 0.005 rad above the
    # surface's plane: lit for shadow(), but outside ang_max = 89 deg (0.0175 rad) for sw_dir_cor (0); east sun: lit
    assert out["code"][:, 0, 0].tolist() == [1, 0, 0]
    assert out["val"][0, 0, 0] == 0 and out["val"][1, 0, 0] == 0 and out["val"][2, 0, 0] > 1.0
    assert np.isinf(out["margin"][0, 0, 0])
    c["mask"][:] = 0
    c["fill"] = -5.0
    out = run(c, [sun(90.0, 0.2)])
    assert out["code"][0, 0, 0] == 3 and out["val"][0, 0, 0] == -5.0


def test_fold_is_float64_ascending_with_one_rounding():
    codes = np.array([0, 2, 0, 1], np.uint8).reshape(4, 1, 1)
    vals = np.array([1.0e8, 1.0, -1.0e8, 0.5], np.float32).reshape(4, 1, 1)
    w = np.array([1.0, 3.0, 1.0, 2.0], np.float32)
    sw, lit = R.fold(codes, vals, w, np.ones((1, 1), np.uint8), np.nan)
    assert sw[0, 0] == 4.0 and lit[0, 0] == 2.0              # a float32 accumulator would lose the 3.0
    sw, lit = R.fold(codes, vals, None, np.zeros((1, 1), np.uint8), -2.0)
    assert sw[0, 0] == -2.0 and lit[0, 0] == -2.0


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_gpu_cases_respect_the_exclusion_cap(name):
    c = R.case(name)
    ref = R.reference(c)
    assert R.inside_margin_share(c, ref) <= R.CAP
    unmasked = ref["code"][:, c["mask"] == 1]
    if unmasked.size >= 100:                                 # the larger cases see every code
        assert all((unmasked == k).any() for k in (0, 1, 2))
    assert (ref["code"][:, c["mask"] != 1] == 3).all()


def test_gpu_cases_cover_the_issue():
    assert {c[4] for c in R.CASES} == {1, 2, 7, 360} and {c[5] for c in R.CASES} == {1, 5} and R.CHUNK_TEST < 5
    assert {c[1] for c in R.CASES} == {(37, 53), (1, 1), (1, 130)} and {c[6] for c in R.CASES} == {"planar", "random"}
    c = R.case("inner_A360_planar")                          # due north (ce = 0, cn > 0), the wrap, the zenith
    ci, cj = 37 // 2, 53 // 2
    cell = lambda a: a[ci:ci + 1, cj:cj + 1]
    for idx, want in ((-1, "north"), (-2, "wrap"), (-3, "zenith")):
        s, _, _ = R.setup(c["suns"][idx], cell(c["vert"]), cell(c["vec_norm"]), cell(c["vec_tilt"]))
        _, _, k0, k1, t = (v[0, 0] for v in R.horizon_at(s, cell(c["vec_norm"]), cell(c["vec_north"]), cell(c["hori"])))
        if want == "north":
            assert s[0, 0, 0] == 0.0 and s[0, 0, 1] > 0.0 and (k0, k1, t) == (0, 1, 0.0)
        elif want == "wrap":
            assert (k0, k1) == (359, 0) and t > 0.99
        else:
            assert s[0, 0].tolist() == [0.0, 0.0, 1.0] and (k0, k1, t) == (0, 1, 0.0)
