"""The reference's own ray-casting statements, compiled and executed, against the oracle's restatement of them.

oracle/_ref/libhz_ref.so (oracle/Makefile ``make ref``, front end oracle/ref.py) holds the reference's horizon_comp.cpp
and shadow_comp.cpp, compiled unmodified with its own flags and linked with a stand-in Embree that answers every ray
with the ORACLE's scene and triangle test.  So for one input

    reference driver + oracle intersector     (oracle.ref)
    oracle driver    + oracle intersector     (oracle.oracle)

must agree word for word: every comparison below is equality of bit patterns (NaN = NaN) and of ray counts.  That pins
the oracle's reading of the searches, the index arithmetic with its float / double promotions, the trig tables, the ray
origins, the rotation, the refraction branch and the shadow codes.  What Embree itself would decide for a ray is NOT
pinned here (README.md, tests/embree_pin.py).

Guard cases: ray_guess_const and ray_discrete_sampling of the reference do not return when a ray is still blocked at
the top table index or still free at index 0 (the oracle counts these as "guards" and breaks out).  Every test therefore
asserts ``guards == 0`` on the oracle BEFORE the reference is called on the same input, and the front end runs the
reference under a ray budget on top of that.

Not marked gpu: runs wherever the library is.  Where the reference tree is present the library must be too (a missing
one fails); elsewhere the module skips only if oracle/_ref/libhz_ref.so is absent.
"""
import numpy as np
import pytest

from horayzon_amd import synth
from oracle import ref
from tests import cases


@pytest.fixture(scope="module", autouse=True)
def _library(orc):
    if not ref.available():
        if ref.reference_present():
            pytest.fail("the reference tree is present but oracle/_ref/libhz_ref.so was not built (build() / make -C oracle ref)")
        pytest.skip("no oracle/_ref/libhz_ref.so and no reference tree to build it from")
    ref.lib()
    yield
    orc.set_libm(False)
    orc.set_quad_order(False)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_words(a, b):
    """Equality of bit patterns with every NaN equal to every NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def n_diff(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return int(((bits(a) != bits(b)) & ~(na & nb)).sum())


# ------------------------------------------------------------------------------------------------------------------
# inputs: DEMs of 40 ... 64 vertices a side, rings of 10 ... 20 cells, all free of guard cases (asserted per test)
# ------------------------------------------------------------------------------------------------------------------

def _hill():
    return synth.gaussian_hill(n=56, dx=50.0, height=200.0, sigma=400.0, offset=12)


def _rough(tilt=True):
    return cases.rough_terrain(48, 52, seed=11, dx=30.0, dy=30.0, relief=120.0, offset=10, tilt_frames=tilt)


def _large_coords():
    return cases.rough_terrain(44, 46, seed=5, dx=25.0, dy=25.0, relief=90.0, offset=10, tilt_frames=True,
                               origin=(2.6e6, 1.2e6))


def _inner(g, rows, cols):
    """Case dict `g` with the inner domain cut down to the given row / column slices (frames and offsets follow)."""
    out = dict(g)
    out["vec_norm"] = np.ascontiguousarray(g["vec_norm"][rows, cols])
    out["vec_north"] = np.ascontiguousarray(g["vec_north"][rows, cols])
    out["offset_0"] = g["offset_0"] + rows.start
    out["offset_1"] = g["offset_1"] + cols.start
    return out


def _checker(shape, keep=2):
    i, j = np.indices(shape)
    return ((i + 2 * j) % 3 < keep).astype(np.uint8)


def gridded_both(orc, kw, par, max_factor=2):
    """(oracle result, oracle stats, reference result, reference stats); the oracle goes first and must be guard-free."""
    a, azim_a, so = orc.horizon_gridded(**kw, **par, return_stats=True)
    assert so["guards"] == 0, "guard case: the reference would not return (%d guard events)" % so["guards"]
    b, azim_b, sr = ref.horizon_gridded(**kw, **par, max_rays=max_factor * so["rays"] + 16, return_stats=True)
    assert np.array_equal(bits(azim_a), bits(azim_b))
    return a, so, b, sr


GRID_CASES = {
    "hill": lambda: (cases.grid_kwargs(_hill()), dict(dist_search=1.3)),
    "rough_tilted": lambda: (cases.grid_kwargs(_rough()), dict(dist_search=0.28)),
    "large_coords": lambda: (cases.grid_kwargs(_large_coords()), dict(dist_search=0.24)),
    "mask_fill": lambda: (cases.grid_kwargs(_rough()), dict(dist_search=0.28, mask=_checker((28, 32)), hori_fill=-1.25)),
    "outer_tin": lambda: (cases.grid_kwargs(_rough()), dict(
        dist_search=4.0, **dict(zip(("vert_simp", "num_vert_simp", "tri_ind_simp", "num_tri_simp"),
                                    cases.outer_tin(_rough(), margin=3000.0, zval=300.0))))),
    "one_cell": lambda: (cases.grid_kwargs(_inner(_rough(), slice(13, 14), slice(17, 18))), dict(dist_search=0.28)),
    "one_row": lambda: (cases.grid_kwargs(_inner(_rough(), slice(20, 21), slice(0, 32))), dict(dist_search=0.28)),
}


@pytest.mark.parametrize("alg", cases.ALGS)
@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_horizon_gridded(orc, name, alg):
    """horizon_gridded_comp (horizon_comp.cpp:629-822) with each search (:302-498): horizon words and ray count.
    guards == 0 is asserted on the oracle first (see the module docstring: the reference does not return otherwise)."""
    kw, par = GRID_CASES[name]()
    par = dict(par, azim_num=12 if alg == "discrete_sampling" else 36, ray_algorithm=alg, geom_type="triangle")
    a, so, b, sr = gridded_both(orc, kw, par)
    assert n_diff(a, b) == 0, "%d of %d horizon words differ" % (n_diff(a, b), a.size)
    assert same_words(a, b)
    assert sr["rays"] == so["rays"] == sr["rays_cast"], (sr["rays"], so["rays"], sr["rays_cast"])
    m = par.get("mask")
    if m is not None:
        assert (b[m != 1] == np.float32(-1.25)).all() and (m != 1).any() and (m == 1).any()
    computed = b if m is None else b[m == 1]
    assert np.isfinite(computed).all()
    if computed.size > par["azim_num"]:
        assert np.unique(bits(computed)).size > 8, "horizon is (almost) constant: the comparison would be vacuous"


def test_outer_tin_is_seen(orc):
    """The outer-TIN case is only worth its name if the second geometry changes horizons of the reference's run."""
    kw, par = GRID_CASES["outer_tin"]()
    par = dict(par, azim_num=24, ray_algorithm="binary_search", geom_type="triangle")
    _, _, with_tin, _ = gridded_both(orc, kw, par)
    bare = {k: v for k, v in par.items() if k not in ("vert_simp", "num_vert_simp", "tri_ind_simp", "num_tri_simp")}
    a, _, so = orc.horizon_gridded(**kw, **bare, return_stats=True)
    assert so["guards"] == 0
    without, _ = ref.horizon_gridded(**kw, **bare)
    assert same_words(a, without)
    assert n_diff(with_tin, without) > 0


def _sweep_kw():
    g = synth.gaussian_hill(n=44, dx=50.0, height=160.0, sigma=350.0, offset=14)      # 16 x 16 inner cells
    return cases.grid_kwargs(g)


SWEEP = ([dict(azim_num=n) for n in (1, 4, 6, 45, 360)]
         + [dict(hori_acc=a, elev_ang_low_lim=lo) for a in (0.1, 0.25, 1.0) for lo in (-15.0, -60.0, -89.98)]
         + [dict(ray_org_elev=e) for e in (0.0, 0.1, 2.0)]
         + [dict(ray_org_elev=e, elev_ang_low_lim=-89.98, hori_acc=1.0, azim_num=6) for e in (0.0, 2.0)]
         # (with the default low limit of -15 degrees a 200 m search leaves downhill rays free at index 0: a guard case)
         + [dict(dist_search=0.2, elev_ang_low_lim=-35.0), dict(dist_search=0.2, elev_ang_low_lim=-60.0, azim_num=45)])


def _sweep_id(v):
    return ",".join("%s=%g" % kv for kv in sorted(v.items()))


# ray_org_elev = 0.0 puts the origin ON the surface: every ray is blocked at t = 0 by the cell's own triangles, also at the
# top table index -- a guard case for the two searches that walk the table (test_origin_on_the_surface_is_a_guard_case), so
# the reference can run it with binary_search only
SWEEP_RUNS = [pytest.param(v, a, id=_sweep_id(v) + "-" + a) for v in SWEEP for a in cases.ALGS
              if not (v.get("ray_org_elev") == 0.0 and a != "binary_search")]


@pytest.mark.parametrize("alg", ("guess_constant", "discrete_sampling"))
def test_origin_on_the_surface_is_a_guard_case(orc, alg):
    """Why ray_org_elev = 0.0 is swept with binary_search only: the oracle reports guard events for the other two."""
    _, _, so = orc.horizon_gridded(**_sweep_kw(), dist_search=1.0, azim_num=6, ray_org_elev=0.0, ray_algorithm=alg,
                                   geom_type="triangle", return_stats=True)
    assert so["guards"] > 0


@pytest.mark.parametrize("var,alg", SWEEP_RUNS)
def test_horizon_gridded_parameter_sweep(orc, var, alg):
    """azim_num in {1, 4, 6, 45, 360}, hori_acc in {0.1, 0.25, 1.0} x elev_ang_low_lim in {-15, -60, -89.98} (the table
    sizes and the roundf() index arithmetic), ray_org_elev in {0.0, 0.1, 2.0} (the ray origin), and a dist_search of
    200 m on a 700 m ring so that horizons end at the search distance.  guards == 0 first, as everywhere."""
    kw = _sweep_kw()
    par = dict(dist_search=1.0, azim_num=12, hori_acc=0.25, elev_ang_low_lim=-15.0, ray_org_elev=0.01)
    par.update(var)
    par.update(ray_algorithm=alg, geom_type="triangle")
    if par["azim_num"] == 360 or (alg == "discrete_sampling" and par["hori_acc"] < 0.2):
        par["mask"] = _checker((16, 16), keep=1)                                      # a third of the cells: keeps it quick
    a, so, b, sr = gridded_both(orc, kw, par)
    assert n_diff(a, b) == 0, "%d of %d horizon words differ" % (n_diff(a, b), a.size)
    assert sr["rays"] == so["rays"]
    if "dist_search" in var:       # the short search must matter: some horizon differs from the long search's
        long_, _, so2 = orc.horizon_gridded(**kw, **dict(par, dist_search=1.0), return_stats=True)
        assert n_diff(a, long_) > 0


def test_guard_case_ends_with_an_error_not_a_hang(orc):
    """A steep hill on a narrow ring: rays stay free at table index 0, the oracle counts guard events, the reference's
    loop would not end.  Under the ray budget the call raises instead."""
    g = synth.gaussian_hill(n=40, dx=50.0, height=800.0, sigma=500.0, offset=12)
    kw = cases.grid_kwargs(g)
    par = dict(dist_search=5.0, azim_num=12, ray_algorithm="guess_constant", geom_type="triangle")
    _, _, so = orc.horizon_gridded(**kw, **par, return_stats=True)
    assert so["guards"] > 0
    with pytest.raises(ref.RayBudgetExceeded):
        ref.horizon_gridded(**kw, **par, max_rays=2 * so["rays"])
    # and the library is usable afterwards
    par["ray_algorithm"] = "binary_search"
    a, _ = orc.horizon_gridded(**kw, **par)
    b, _ = ref.horizon_gridded(**kw, **par)
    assert same_words(a, b)


@pytest.mark.parametrize("geom", ("quad", "grid"))
def test_quad_and_grid_geometry_under_the_quad_order_model(orc, geom):
    """'quad' / 'grid' hand Embree quads; the oracle models their second triangle through orc_set_quad_order(1).  The
    stand-in checks the reference's quad index buffer / RTCGrid and refuses the combination the oracle does not model."""
    kw, par = GRID_CASES["rough_tilted"]()
    par = dict(par, azim_num=12, ray_algorithm="guess_constant", geom_type=geom)
    with pytest.raises(ref.StandinError):
        ref.horizon_gridded(**kw, **par)
    orc.set_quad_order(True)
    try:
        a, so, b, sr = gridded_both(orc, kw, par)
        with pytest.raises(ref.StandinError):
            ref.horizon_gridded(**kw, **dict(par, geom_type="triangle"))
    finally:
        orc.set_quad_order(False)
    assert n_diff(a, b) == 0 and sr["rays"] == so["rays"]


# ------------------------------------------------------------------------------------------------------------------
# trig tables (horizon_comp.cpp:711-731): read off the directions of the rays the reference casts
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("azim_num,hori_acc,low", [(45, 0.25, -15.0), (360, 0.25, -15.0), (6, 0.1, -60.0),
                                                   (4, 1.0, -89.98), (7, 0.3, -33.3)])
def test_tables_from_the_rays_the_reference_casts(orc, azim_num, hori_acc, low):
    """With planar frames rot_inv is the identity, so a ray's direction IS (elev_cos[i] azim_sin[k], elev_cos[i]
    azim_cos[k], elev_sin[i]) of the reference's tables (:318-320, :55-62; adding the 0 * x terms is exact).  Every ray the
    reference casts is recorded by the stand-in and must be such a product of oracle.tables() entries -- which float
    overload sin(ang) / cos(ang) resolve to, the rounding of `ang` to float before the call, elev_num -- and its tfar the
    table's search distance in metres.  All azimuth entries occur; the elevation entries that occur are those the
    searches visit (binary search and guess_constant over rough terrain: hundreds of distinct indices)."""
    kw = cases.grid_kwargs(_rough(tilt=False))
    tab = orc.tables(azim_num, hori_acc, low, 0.28)
    es, ec, asn, acs = tab["elev_sin"], tab["elev_cos"], tab["azim_sin"], tab["azim_cos"]
    assert np.unique(es).size == es.size          # elev_sin identifies the table index
    seen_e, seen_a, n_rays = set(), set(), 0
    for alg in ("binary_search", "guess_constant"):
        par = dict(dist_search=0.28, azim_num=azim_num, hori_acc=hori_acc, elev_ang_low_lim=low, ray_algorithm=alg,
                   geom_type="triangle", mask=_checker((28, 32), keep=1))
        _, _, so = orc.horizon_gridded(**kw, **par, return_stats=True)
        assert so["guards"] == 0
        _, _, sr = ref.horizon_gridded(**kw, **par, max_rays=2 * so["rays"], record=so["rays"], return_stats=True)
        rec = sr["recorded"]
        assert rec.shape[0] == so["rays"] == sr["rays"]
        assert (bits(rec[:, 6]) == bits(np.float32(tab["dist"]))).all() and (rec[:, 7] == 0).all()
        d = np.unique(rec[:, 3:6] + np.float32(0.0), axis=0)          # + 0: -0 -> +0, as adding the 0 * x terms does
        order = np.argsort(es)
        pos = np.searchsorted(es[order], d[:, 2])
        assert (pos < es.size).all() and (es[order][np.minimum(pos, es.size - 1)] == d[:, 2]).all(), \
            "a ray's z component is not an elev_sin entry of oracle.tables()"
        i = order[pos]
        cand_x = (ec[i][:, None] * asn[None, :]) + np.float32(0.0)
        cand_y = (ec[i][:, None] * acs[None, :]) + np.float32(0.0)
        match = (cand_x == d[:, 0:1]) & (cand_y == d[:, 1:2])
        assert match.any(axis=1).all(), "%d ray directions are not products of oracle.tables() entries" % int((~match.any(axis=1)).sum())
        seen_e.update(i.tolist())
        seen_a.update(np.nonzero(match.any(axis=0))[0].tolist())
        n_rays += rec.shape[0]
    assert seen_a == set(range(azim_num))
    assert len(seen_e) > min(100, tab["elev_num"] // 4), (len(seen_e), tab["elev_num"])


# ------------------------------------------------------------------------------------------------------------------
# horizon_locations (horizon_comp.cpp:828-1094)
# ------------------------------------------------------------------------------------------------------------------

def _locations():
    """Locations on vertices, on cell edges, in cell interiors, above and below the surface, one far outside the DEM
    (never finds the surface: its rows stay NaN), each with its own frame and ray_org_elev."""
    g = _rough(tilt=False)
    x, y, z = g["x"].astype(np.float64), g["y"].astype(np.float64), g["z"].astype(np.float64)
    pts = []
    for (i, j, fi, fj, dz) in [(20, 24, 0.0, 0.0, 0.0), (14, 30, 0.0, 0.0, 7.0), (27, 18, 0.0, 0.0, -3.0),       # vertices
                               (18, 22, 0.5, 0.0, 4.0), (22, 26, 0.0, 0.25, -2.0), (25, 21, 0.75, 0.0, 0.0),     # edges
                               (16, 19, 0.3, 0.6, 5.0), (23, 28, 0.7, 0.2, -4.0), (21, 23, 0.5, 0.5, 1.0),       # interior
                               (19, 25, 0.1, 0.1, 60.0)]:                                                        # well above
        px = x[j] + fj * (x[j + 1] - x[j]); py = y[i] + fi * (y[i + 1] - y[i])
        zz = (z[i, j] * (1 - fi) * (1 - fj) + z[i + 1, j] * fi * (1 - fj) + z[i, j + 1] * (1 - fi) * fj
              + z[i + 1, j + 1] * fi * fj)
        pts.append((px, py, zz + dz))
    pts.append((x[-1] + 500.0, y[0] + 500.0, 300.0))                                                           # outside
    coords = np.array(pts, np.float32)
    n = coords.shape[0]
    rng = np.random.default_rng(3)
    tilt = np.deg2rad(1.5) * rng.random(n); dirn = rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.sin(tilt) * np.cos(dirn), np.sin(tilt) * np.sin(dirn), np.cos(tilt)], axis=1)
    north = np.array([0.0, 1.0, 0.0])[None, :] - nrm[:, 1:2] * nrm
    north /= np.linalg.norm(north, axis=1, keepdims=True)
    roe = np.linspace(0.01, 2.5, n).astype(np.float32)
    return g, coords, np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(north, np.float32), roe


@pytest.mark.parametrize("dist_out", (False, True))
@pytest.mark.parametrize("alg", cases.ALGS)
def test_horizon_locations(orc, alg, dist_out):
    """The surface snap along +/- normal (rtcIntersect1, tfar 100 km, `dist *= -1.0`), the origin `ini + norm * (dist +
    ray_org_elev[i])`, the searches, and with hori_dist_out the rtcIntersect1 variants of the searches (:519-612).
    guards == 0 first (module docstring).  guess_constant has no distance variant: both sides refuse it."""
    g, coords, nrm, north, roe = _locations()
    args = (g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], coords, nrm, north)
    par = dict(dist_search=0.28, azim_num=24 if alg == "discrete_sampling" else 60, hori_acc=0.25, ray_algorithm=alg,
               geom_type="triangle", elev_ang_low_lim=-25.0, ray_org_elev=roe, hori_dist_out=dist_out)
    if dist_out and alg == "guess_constant":
        for mod in (orc, ref):
            with pytest.raises(TypeError):
                mod.horizon_locations(*args, **par)
        return
    out_a = orc.horizon_locations(*args, **par, return_stats=True)
    so = out_a[-1]
    assert so["guards"] == 0
    out_b = ref.horizon_locations(*args, **par, max_rays=2 * so["rays"] + 4 * len(roe), return_stats=True)
    sr = out_b[-1]
    for a, b in zip(out_a[:-1], out_b[:-1]):
        assert n_diff(a, b) == 0
    assert sr["rays"] == so["rays"]
    n = coords.shape[0]
    assert so["found"] == n - 1
    assert n - 1 <= sr["rays_cast"] - sr["rays"] <= 2 * (n - 1) + 2        # one or two surface rays per location
    hori = out_b[0]
    assert np.isnan(hori[-1]).all() and np.isfinite(hori[:-1]).all()
    assert np.unique(bits(hori[:-1])).size > 8
    if dist_out:
        dist = out_b[1]
        assert np.isnan(dist[-1]).all() and np.isfinite(dist[:-1]).all() and (dist[:-1] > 0).any()


@pytest.mark.parametrize("alg", ("binary_search", "discrete_sampling"))
def test_horizon_locations_last_hit_distance_persists(orc, alg):
    """dist_hit lives outside the azimuth loop (:526-527, :570-571): an azimuth whose rays all miss reports the distance of
    the last hit of an EARLIER azimuth (0.0 before any hit).  A location high above a summit, a low limit of -8 degrees
    and a 150 m search: most azimuths see nothing.  discrete_sampling ends on its first free ray, so guards stay 0."""
    g = _rough(tilt=False)
    z = g["z"]
    i, j = np.unravel_index(np.argmax(z[12:36, 12:40]), (24, 28)); i += 12; j += 12
    coords = np.array([[g["x"][j], g["y"][i], z[i, j] + 30.0], [g["x"][j + 3], g["y"][i + 2], z[i + 2, j + 3] + 1.0]], np.float32)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (2, 1)); north = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (2, 1))
    args = (g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], coords, nrm, north)
    par = dict(dist_search=0.15, azim_num=72, hori_acc=0.25, ray_algorithm=alg, geom_type="triangle",
               elev_ang_low_lim=-8.0, ray_org_elev=np.array([30.0, 0.5], np.float32), hori_dist_out=True)
    ha, da, _, so = orc.horizon_locations(*args, **par, return_stats=True)
    assert so["guards"] == 0
    hb, db, _, sr = ref.horizon_locations(*args, **par, max_rays=2 * so["rays"] + 8, return_stats=True)
    assert n_diff(ha, hb) == 0 and n_diff(da, db) == 0 and sr["rays"] == so["rays"]
    rep = bits(db[:, 1:]) == bits(db[:, :-1])
    assert rep.any(), "no azimuth repeats its predecessor's distance: the persistence is not exercised"
    assert (~rep).any()


# ------------------------------------------------------------------------------------------------------------------
# Terrain.shadow / sw_dir_cor (shadow_comp.cpp:304-605)
# ------------------------------------------------------------------------------------------------------------------

def _terrain_case():
    g = synth.gaussian_hill(n=60, dx=50.0, height=900.0, sigma=450.0, offset=10)     # 40 x 40 inner cells
    vec_tilt, vec_norm, enl, elev, mask = cases.terrain_inputs(g)
    mask = _checker(mask.shape)
    # elevations from below sea level to 8 km for the pressure formula (they enter the refraction only)
    elev = np.linspace(-420.0, 8000.0, elev.size, dtype=np.float32).reshape(elev.shape)
    return g, (g["vert_grid"], 60, 60, 10, 10, vec_tilt, vec_norm, enl, elev, mask)


def _suns(g):
    c = np.array([g["x"].mean(), g["y"].mean(), 0.0])
    def at(az_deg, el_deg, r=1.0e8):
        az, el = np.deg2rad(az_deg), np.deg2rad(el_deg)
        return (c + r * np.array([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)])).astype(np.float32)
    return {"high": at(160.0, 62.0), "all_codes": at(245.0, 9.0), "grazing": at(95.0, 1.2), "grazing2": at(310.0, 0.4),
            "below": at(20.0, -6.0), "near": at(200.0, 25.0, r=4.0e3)}


def _terrain_both(orc, args, **kw):
    ta, tb = orc.Terrain(), ref.Terrain()
    ta.initialise(*args, geom_type="triangle", **kw)
    tb.initialise(*args, geom_type="triangle", **kw)
    return ta, tb


def _run_both(ta, tb, sun, shape):
    sa = np.full(shape, 255, np.uint8); sb = sa.copy()
    ta.shadow(sun, sa); tb.shadow(sun, sb)
    rays = (ta.rays, tb.rays)
    fa = np.full(shape, 7.0, np.float32); fb = fa.copy()
    ta.sw_dir_cor(sun, fa); tb.sw_dir_cor(sun, fb)
    return sa, sb, fa, fb, rays + (ta.rays, tb.rays)


@pytest.mark.parametrize("ang_max", (89.0, 55.0))
@pytest.mark.parametrize("fill", (np.nan, -3.5))
def test_terrain_without_refraction(orc, fill, ang_max):
    """shadow() and sw_dir_cor() (:386-605) in the oracle's default mode: origin, vec_unit (the sqrt overload), the two
    dot products, `> 0.0` and `> dot_prod_min = cos(deg2rad(ang_max))`, the clamp of dot_prod_ns, the codes 0 ... 3 and
    the fill value; the count of rays cast as well."""
    g, args = _terrain_case()
    ta, tb = _terrain_both(orc, args, sw_dir_cor_fill=fill, ang_max=ang_max)
    shape = args[-1].shape
    seen, lit = set(), 0
    for name, sun in _suns(g).items():
        sa, sb, fa, fb, rays = _run_both(ta, tb, sun, shape)
        assert np.array_equal(sa, sb), name
        assert n_diff(fa, fb) == 0, name
        assert rays[0] == rays[1] and rays[2] == rays[3], (name, rays)
        seen.update(np.unique(sb).tolist())
        lit += int((fb[args[-1] == 1] > 0).sum())
        if name == "all_codes":
            assert set(np.unique(sb).tolist()) == {0, 1, 2, 3}
        m = args[-1] != 1
        assert (np.isnan(fb[m]).all() if np.isnan(fill) else (fb[m] == np.float32(fill)).all())
    assert seen == {0, 1, 2, 3} and lit > 100


@pytest.mark.parametrize("ang_max", (89.0, 55.0))
def test_terrain_with_refraction_platform_libm(orc, ang_max):
    """The refraction branch (:135-159, :430-446): acos, pow, tan, cos, sin of the platform's FLOAT libm (the overloads the
    reference's calls resolve to), the double-precision constants in between, the order of the operations, the clamp of the
    true elevation to [-1, 90].  The oracle in set_libm(1) mode calls the same platform routines: bit for bit."""
    g, args = _terrain_case()
    ta, tb = _terrain_both(orc, args, sw_dir_cor_fill=-9.0, ang_max=ang_max, refrac_cor=True)
    _, tn = _terrain_both(orc, args, sw_dir_cor_fill=-9.0, ang_max=ang_max, refrac_cor=False)
    shape = args[-1].shape
    orc.set_libm(1)
    try:
        changed = 0
        for name, sun in _suns(g).items():
            sa, sb, fa, fb, rays = _run_both(ta, tb, sun, shape)
            assert np.array_equal(sa, sb), name
            assert n_diff(fa, fb) == 0, (name, n_diff(fa, fb))
            assert rays[0] == rays[1] and rays[2] == rays[3]
            fn = np.full(shape, 7.0, np.float32); tn.sw_dir_cor(sun, fn)
            changed += n_diff(fb, fn)
    finally:
        orc.set_libm(False)
    assert changed > 100, "refraction changes (almost) no sw_dir_cor word: the branch is not exercised"


def test_the_comparison_sees_last_bit_changes(orc):
    """Not vacuous: with refraction on and the oracle left in its default mode (hz_crmath.h, correctly rounded) the
    reference -- platform libm -- must differ from it in some sw_dir_cor words on this input, and agree again under
    set_libm(1).  So the equality above is a statement about last bits, not about a comparison that cannot fail."""
    g, args = _terrain_case()
    ta, tb = _terrain_both(orc, args, sw_dir_cor_fill=-9.0, refrac_cor=True)
    shape = args[-1].shape
    diff0 = diff1 = 0
    for name, sun in _suns(g).items():
        fb = np.full(shape, 7.0, np.float32); tb.sw_dir_cor(sun, fb)
        f0 = fb.copy(); ta.sw_dir_cor(sun, f0)
        orc.set_libm(1)
        try:
            f1 = fb.copy(); ta.sw_dir_cor(sun, f1)
        finally:
            orc.set_libm(False)
        diff0 += n_diff(fb, f0); diff1 += n_diff(fb, f1)
    print("sw_dir_cor words differing from the reference: %d with hz_crmath.h, %d with the platform libm" % (diff0, diff1))
    assert diff1 == 0
    assert diff0 > 0
