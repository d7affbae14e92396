"""The NumPy reference of the horizon reductions (tests/topo_reference.py) is pinned to what the real program wrote
(tests/golden/svf_reference.npz), to the C oracle and to closed forms -- before any kernel is held to it
(tests/test_gpu_topo_reference.py).  No GPU."""
import os

import numpy as np
import pytest

from tests import cases
from tests import topo_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svf_reference.npz")
ULP32_AT_HALF = float(np.spacing(np.float32(0.5)))          # 5.96e-8: one float32 ulp of a value in [0.5, 1)


@pytest.mark.parametrize("n", "abc")
def test_contract_equals_reference_made_fixtures(n):
    """SVF and openness bit for bit.  VSF within one float32 ulp in at most 10 % of the cells (measured 2.0 %, 6.3 % and
    0 % for a, b, c: the reference's own build passes -ffast-math, which lets its compiler rearrange 1 - cos(pi/2 - h))."""
    d = np.load(GOLDEN)
    ref = R.topo_reference(d["azim_" + n], d["hori_" + n], d["tilt_" + n])
    assert ref["svf"].contract.tobytes() == d["svf_" + n].tobytes()
    assert ref["openness"].contract.tobytes() == d["top_" + n].tobytes()
    vsf, gold = ref["vsf"].contract, d["vsf_" + n]
    differ = vsf != gold
    print("case %s: VSF differs in %.1f %% of the cells, max %.3g" % (n, 100.0 * differ.mean(), np.abs(vsf - gold).max()))
    assert differ.mean() <= 0.10
    assert float(gold.max()) < 1.0 and np.abs(vsf.astype(np.float64) - gold).max() <= ULP32_AT_HALF


def test_contract_equals_oracle_on_rough_terrain(orc):
    """orc.sky_view_factor (C, the loop of topo_param.pyx:412-460) on a real horizon of 72 x 72 cells of rough terrain."""
    g = cases.rough_terrain(80, 80, seed=7, offset=4)
    kw = cases.grid_kwargs(g)
    tilt, *_ = cases.terrain_inputs(g)
    hori, azim = orc.horizon_gridded(**kw, dist_search=2.0, azim_num=36)
    assert hori.shape == (72, 72, 36)
    ref = R.topo_reference(azim, hori, tilt, which="svf")["svf"]
    assert ref.contract.tobytes() == orc.sky_view_factor(azim, hori, tilt).tobytes()


def _acc_bound(res, A):
    """What `contract` may be off by at most: A float32 roundings of the accumulator (half an ulp of its largest value
    each), scaled to the output, and the rounding of the output itself."""
    return 0.5 * A * float(np.spacing(res.agg_max.max())) * res.scale + float(np.spacing(np.abs(res.contract).max()))


def test_closed_forms():
    d = np.load(GOLDEN)
    rng = np.random.default_rng(11)
    shape = (2, 2)
    for A in (2, 36, 360):
        azim = R.make_azim(A)
        eps = A * 1.0e-7                                    # the spacing float32(2 pi / A) times A is 2 pi to 6e-8 relative
        # a flat horizon under the normal (0, 0, 1): SVF and VSF are 1
        flat = np.zeros(shape + (A,), np.float32)
        ref = R.topo_reference(azim, flat, R.tilt_up(shape))
        for name in ("svf", "vsf"):
            assert np.abs(ref[name].exact - 1.0).max() <= eps
            assert np.abs(ref[name].contract - 1.0).max() <= eps + _acc_bound(ref[name], A)
        # a uniform 30 degree horizon: SVF = cos^2(30 deg), VSF = 1 - sin(30 deg)
        h30 = np.full(shape + (A,), np.deg2rad(30.0), np.float32)
        ref = R.topo_reference(azim, h30, R.tilt_up(shape))
        assert np.abs(ref["svf"].exact - 0.75).max() <= eps + 1e-7       # float32(pi / 6) is 3e-8 off
        assert np.abs(ref["vsf"].exact - 0.5).max() <= eps + 1e-7
        assert np.abs(ref["svf"].contract - 0.75).max() <= eps + 1e-7 + _acc_bound(ref["svf"], A)
        assert np.abs(ref["vsf"].contract - 0.5).max() <= eps + 1e-7 + _acc_bound(ref["vsf"], A)
        # openness of a constant horizon h is pi / 2 - h
        for hval in (-0.3, 0.0, 1.2):
            hc = np.full(shape + (A,), hval, np.float32)
            top = R.topo_reference(azim, hc, which="openness")["openness"]
            assert np.abs(top.exact - (np.pi / 2.0 - np.float64(np.float32(hval)))).max() <= 1e-15
            assert np.abs(top.contract - (np.pi / 2.0 - hval)).max() <= 6e-8 + _acc_bound(top, A)
    # a unit normal of slope s above a flat horizon: the plane cuts the dome, SVF = (1 + cos s) / 2 (the azimuth sum is a
    # rectangle rule on a function with a kink where the plane crosses the horizon: 1e-5 at 1440 azimuths)
    azim = R.make_azim(1440)
    tilt = R.tilt_slopes(rng, (1, 8), 60.0)
    ref = R.topo_reference(azim, np.zeros((1, 8, 1440), np.float32), tilt, which="svf")["svf"]
    assert np.abs(ref.exact - (1.0 + tilt[..., 2].astype(np.float64)) / 2.0).max() <= 1e-5
    # the fixtures made by the reference for exactly these two set-ups
    azim = d["azim_a"]
    A = len(azim)
    ref = R.topo_reference(azim, np.zeros(shape + (A,), np.float32), R.tilt_up(shape), which="svf")["svf"]
    assert ref.contract.tobytes() == d["svf_flat"].tobytes()
    ref = R.topo_reference(azim, np.full(shape + (A,), np.deg2rad(30.0), np.float32), R.tilt_up(shape), which="svf")["svf"]
    assert ref.contract.tobytes() == d["svf_30deg"].tobytes()


# (azimuths, largest slope [degree], E_ref measured when this was written: max |contract - exact| over SVF and VSF)
E_REF_CLASSES = ((36, 35.0, 2.7e-7), (360, 50.0, 7.2e-7), (1440, 70.0, 1.2e-6), (3456, 60.0, 1.6e-6))


@pytest.mark.parametrize("A,slope,measured", E_REF_CLASSES)
def test_contract_and_exact_differ_by_the_float32_accumulator(A, slope, measured):
    """E_ref = max |contract - exact| is what a float32 accumulator costs: every one of the A additions rounds a sum of up
    to `agg_max` to float32 (half an ulp each), the errors add like a random walk, and the sum is scaled to the output.
    A roundings uniform in +-ulp/2 have a standard deviation of sqrt(A / 12) ulps; `walk` = sqrt(A) / 2 ulps is 1.7 of
    those.  The upper bound is 4 walks (7 standard deviations; the largest of 512 cells is expected near 2 walks) plus the
    float32 rounding of the output and of the azimuths' sine / cosine (6e-8 each), and E_ref must not be an order of
    magnitude below a walk either (a reference that rounds nowhere pins nothing)."""
    rng = np.random.default_rng(100 + A)
    shape = (8, 64)
    azim = R.make_azim(A)
    ref = R.topo_reference(azim, R.hori_uniform(rng, shape, A), R.tilt_slopes(rng, shape, slope))
    for name in R.NAMES:
        res = ref[name]
        e = R.e_ref(res)
        ulp = float(np.spacing(res.agg_max.max())) * res.scale
        walk = 0.5 * np.sqrt(A) * ulp
        worst = 4.0 * walk + 1.2e-7 + float(np.spacing(np.float32(np.abs(res.contract).max())))
        print("A %d slope <= %g %s: E_ref %.3g (walk %.3g, bound %.3g; SVF / VSF when written: %.2g)"
              % (A, slope, name, e, walk, worst, measured))
        assert e <= worst, name
        assert e >= 0.1 * walk, name


def test_perturbing_the_terms_moves_almost_no_cell():
    """+-2 float64 ulps on every term of `contract` (what another libm may differ by) change a float32 sum only where it
    lands within that of a rounding boundary: the share of such cells is what the one-lane-per-cell kernels, which keep the
    reference's float64 terms, may differ from `contract` in (tests/test_gpu_topo_reference.py)."""
    rng = np.random.default_rng(5)
    shape, A = (100, 200), 36
    azim = R.make_azim(A)
    hori, tilt = R.hori_uniform(rng, shape, A), R.tilt_slopes(rng, shape, 70.0)
    ref = R.topo_reference(azim, hori, tilt, which=("svf", "vsf"))
    per = R.topo_reference(azim, hori, tilt, which=("svf", "vsf"), perturb_ulps=2, seed=1)
    for name in ("svf", "vsf"):
        share = float((ref[name].contract != per[name].contract).mean())
        print("%s: %.2g of the cells change" % (name, share))
        assert share <= 1.0e-4


def test_nan_and_degenerate_inputs_of_the_reference():
    """What the reference program does with them, so that the kernels can be held to it: a NaN horizon entry fails
    `hori >= hori_plane` and the plane's own horizon is taken (SVF and VSF stay numbers), openness turns NaN; a tilt with
    tz == 0 gives the plane's horizon +-pi/2 where both quotients are infinite of opposite sign, NaN where they cancel."""
    A = 8
    azim = R.make_azim(A, start=0.1)
    hori = np.full((1, 2, A), 0.2, np.float32)
    hori[0, 1, 3] = np.nan
    ref = R.topo_reference(azim, hori, R.tilt_up((1, 2)))
    assert not np.isnan(ref["svf"].contract).any() and not np.isnan(ref["vsf"].contract).any()
    assert np.isnan(ref["openness"].contract).tolist() == [[False, True]]
    assert np.isnan(ref["openness"].exact).tolist() == [[False, True]]
    sector = np.linspace(0.1, 1.4, 12).astype(np.float32)                  # sine and cosine positive throughout
    tilt = np.array([[[0.6, 0.8, 0.0], [-0.6, -0.8, 0.0], [0.6, -0.8, 0.0], [0.6, 0.0, 0.0]]], np.float32)
    ref = R.topo_reference(sector, np.full((1, 4, 12), 0.2, np.float32), tilt)
    for name in ("svf", "vsf"):
        assert np.isnan(ref[name].contract).tolist() == [[False, False, True, True]], name
        assert np.isnan(ref[name].exact).tolist() == [[False, False, True, True]], name
    assert np.abs(ref["vsf"].contract[0, 1]) <= 1e-7                       # the plane hides the whole sector: 1 - sin(pi/2)
