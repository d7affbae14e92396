"""The GPU library against the reference's own compiled driver (oracle/_ref/libhz_ref.so; see tests/test_ref_driver.py and
oracle/ref.py): the reference's statements, executed, on the oracle's intersector -- without the oracle's restatement of
those statements in between.  Reads oracle/_ref/ only, never the reference tree.

Guard cases: the reference does not return on them (tests/test_ref_driver.py, module docstring), so each input is first
run through the oracle, which must report guards == 0; the GPU result must report guard_events == 0 as well.
"""
import numpy as np
import pytest

from horayzon_amd import synth
from oracle import ref
from tests import cases
from tests.test_ref_driver import _checker, _locations, _suns, _terrain_case, bits, n_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library(orc):
    if not ref.available():
        if ref.reference_present():
            pytest.fail("the reference tree is present but oracle/_ref/libhz_ref.so was not built (build() / make -C oracle ref)")
        pytest.skip("no oracle/_ref/libhz_ref.so and no reference tree to build it from")
    ref.lib()
    yield
    orc.set_libm(False)


N0, N1, RING = 37 + 2 * 16, 29 + 2 * 16, 16          # 37 x 29 inner cells, 16-cell ring


def _hill_rect():
    x = (np.arange(N1) * 50.0).astype(np.float32)
    y = ((N0 - 1 - np.arange(N0)) * 50.0).astype(np.float32)
    xx, yy = np.meshgrid(x, y)
    z = (230.0 * np.exp(-((xx - x.mean() - 60.0) ** 2 + (yy - y.mean() + 35.0) ** 2) / (2.0 * 420.0 ** 2))).astype(np.float32)
    vec_norm, vec_north = synth.planar_frames(N0 - 2 * RING, N1 - 2 * RING)
    return dict(vert_grid=synth.pack_vertices(xx, yy, z), dem_dim_0=N0, dem_dim_1=N1, vec_norm=vec_norm,
                vec_north=vec_north, offset_0=RING, offset_1=RING), 1.5


def _rough_tilted():
    g = cases.rough_terrain(N0, N1, seed=23, dx=30.0, dy=30.0, relief=140.0, offset=RING, tilt_frames=True)
    return cases.grid_kwargs(g), 0.45


@pytest.mark.parametrize("azim_num", (6, 360))
@pytest.mark.parametrize("alg", cases.ALGS)
@pytest.mark.parametrize("case", (_hill_rect, _rough_tilted), ids=("hill", "rough_tilted"))
def test_horizon_gridded_against_the_reference_driver(hip, orc, case, alg, azim_num):
    """hori words and num_rays of hz.horizon.horizon_gridded = the reference's horizon_gridded_comp on the same input.
    At 360 azimuths binary_search and discrete_sampling run on a third of the cells (mask), discrete_sampling with
    hori_acc = 1 degree: the reference is serial here and a case has a few seconds."""
    kw, dist = case()
    par = dict(dist_search=dist, azim_num=azim_num, ray_algorithm=alg, geom_type="triangle")
    if azim_num == 360 and alg != "guess_constant":
        par["mask"] = _checker((37, 29), keep=1)
        par["hori_fill"] = -0.5
        if alg == "discrete_sampling":
            par["hori_acc"] = 1.0
    _, _, so = orc.horizon_gridded(**kw, **par, return_stats=True)
    assert so["guards"] == 0, "guard case: the reference would not return"
    want, azim_want, sr = ref.horizon_gridded(**kw, **par, max_rays=2 * so["rays"] + 16, return_stats=True)
    got, azim = hip.horizon.horizon_gridded(**kw, **par)
    st = hip.horizon.last_stats
    assert st["guard_events"] == 0
    assert np.array_equal(bits(azim), bits(azim_want))
    assert n_diff(got, want) == 0, "%d of %d horizon words differ" % (n_diff(got, want), want.size)
    assert st["num_rays"] == sr["rays"], (st["num_rays"], sr["rays"])
    assert np.unique(bits(want)).size > 8


@pytest.mark.parametrize("dist_out", (False, True))
@pytest.mark.parametrize("alg", ("binary_search", "discrete_sampling", "guess_constant"))
def test_horizon_locations_against_the_reference_driver(hip, orc, alg, dist_out):
    """horizon_locations with and without distances (guess_constant has no distance variant: refused on both sides)."""
    g, coords, nrm, north, roe = _locations()
    args = (g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], coords, nrm, north)
    par = dict(dist_search=0.28, azim_num=24 if alg == "discrete_sampling" else 60, hori_acc=0.25, ray_algorithm=alg,
               geom_type="triangle", elev_ang_low_lim=-25.0, ray_org_elev=roe, hori_dist_out=dist_out)
    if dist_out and alg == "guess_constant":
        for f in (hip.horizon.horizon_locations, ref.horizon_locations):
            with pytest.raises(TypeError):
                f(*args, **par)
        return
    so = orc.horizon_locations(*args, **par, return_stats=True)[-1]
    assert so["guards"] == 0, "guard case: the reference would not return"
    want = ref.horizon_locations(*args, **par, max_rays=2 * so["rays"] + 4 * len(roe), return_stats=True)
    got = hip.horizon.horizon_locations(*args, **par)
    st = hip.horizon.last_stats
    assert st["guard_events"] == 0
    for a, b in zip(got, want[:-1]):
        assert n_diff(a, b) == 0
    assert st["num_rays"] == want[-1]["rays"]
    assert np.isnan(want[0][-1]).all() and np.isfinite(want[0][:-1]).all()
    if dist_out:
        assert np.isfinite(want[1][:-1]).all() and np.isnan(want[1][-1]).all()


@pytest.mark.parametrize("ang_max", (89.0, 85.0))
def test_terrain_without_refraction_against_the_reference_driver(hip, ang_max):
    """Terrain.shadow / sw_dir_cor without refraction: equality with the reference's CppTerrain (85 degrees is the
    smallest ang_max the library's argument check, the reference's own, admits)."""
    g, args = _terrain_case()
    tg, tr = hip.shadow.Terrain(), ref.Terrain()
    tg.initialise(*args, geom_type="triangle", sw_dir_cor_fill=-3.5, ang_max=ang_max)
    tr.initialise(*args, geom_type="triangle", sw_dir_cor_fill=-3.5, ang_max=ang_max)
    shape = args[-1].shape
    seen = set()
    for name, sun in _suns(g).items():
        sg = np.full(shape, 255, np.uint8); sr = sg.copy()
        tg.shadow(sun, sg); tr.shadow(sun, sr)
        assert (tg.last_stats or {}).get("guard_events", 0) == 0
        fg = np.full(shape, 7.0, np.float32); fr = fg.copy()
        tg.sw_dir_cor(sun, fg); tr.sw_dir_cor(sun, fr)
        assert np.array_equal(sg, sr), name
        assert n_diff(fg, fr) == 0, name
        seen.update(np.unique(sr).tolist())
    assert seen == {0, 1, 2, 3}


def test_terrain_with_refraction_against_the_reference_driver(hip):
    """With refraction the GPU's contract is the correctly rounded libm (hz_crmath.h), the reference's the platform's:
    a tolerance, in the form and with the bounds of test_gpu_parity.py::test_refraction_against_platform_libm -- at most
    1e-3 of the shadow codes differ, and where they agree sw_dir_cor agrees to 1e-4 relative to max(|reference|, 1)."""
    g, args = _terrain_case()
    tg, tr = hip.shadow.Terrain(), ref.Terrain()
    tg.initialise(*args, geom_type="triangle", refrac_cor=True, sw_dir_cor_fill=-9.0)
    tr.initialise(*args, geom_type="triangle", refrac_cor=True, sw_dir_cor_fill=-9.0)
    shape = args[-1].shape
    n, flips, worst = 0, 0, 0.0
    for name, sun in _suns(g).items():
        sg = np.full(shape, 255, np.uint8); sr = sg.copy()
        tg.shadow(sun, sg); tr.shadow(sun, sr)
        fg = np.full(shape, np.nan, np.float32); fr = fg.copy()
        tg.sw_dir_cor(sun, fg); tr.sw_dir_cor(sun, fr)
        same = sg == sr
        n += sg.size; flips += int((~same).sum())
        if same.any():
            d = np.abs(fg[same] - fr[same]) / np.maximum(np.abs(fr[same]), 1.0)
            worst = max(worst, float(d.max()))
    print("refraction, GPU against the reference driver: %d of %d shadow codes differ (share %.3g), worst relative "
          "sw_dir_cor difference %.3g" % (flips, n, flips / n, worst))
    assert flips <= 1e-3 * n, (flips, n)
    assert worst <= 1e-4, worst
