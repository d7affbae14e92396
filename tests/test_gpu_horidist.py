"""The distance to the horizon of a gridded horizon on the GPU (horizon.horizon_distance, horizon_gridded(hori_dist=True);
hz_horidist.hip) against the CPU reference on the oracle's horizon (tests/horidist_reference.py; DESIGN.md section 4,
clause 16).  Every comparison is equality of all 32-bit words, NaN positions included."""
import functools

import numpy as np
import pytest

from tests import cases
from tests import horidist_reference as ref

pytestmark = pytest.mark.gpu


def _case(name):
    """(grid kwargs, parameters of the horizon, keyword arguments of the outer TIN)"""
    tin = {}
    if name.startswith("a_"):
        g = cases.rough_terrain(48, 48, seed=7, offset=6)
        par = dict(azim_num=24, dist_search=2.0, ray_algorithm=name[2:])
    elif name == "b_tin":
        g = cases.rough_terrain(40, 40, seed=3, offset=4)
        vs, nvs, ts, nts = cases.outer_tin(g)
        tin = dict(vert_simp=vs, num_vert_simp=nvs, tri_ind_simp=ts, num_tri_simp=nts)
        par = dict(azim_num=16, dist_search=8.0)
    elif name == "c_tilted":
        g = cases.rough_terrain(40, 44, seed=11, offset=5, tilt_frames=True)
        par = dict(azim_num=36, dist_search=2.0, hori_acc=1.0, elev_ang_low_lim=-30.0)
    elif name == "d_7_azimuths":          # inner 12 x 63: partial blocks, rows of 7 values
        g = cases.rough_terrain(20, 71, seed=5, offset=4)
        par = dict(azim_num=7, dist_search=2.0, hori_acc=0.15)
    elif name == "d_1_azimuth":
        g = cases.rough_terrain(20, 71, seed=5, offset=4)
        par = dict(azim_num=1, dist_search=2.0, ray_algorithm="binary_search", elev_ang_low_lim=-89.98)
    elif name == "d_13x65":               # inner 13 x 65: one row and one column beyond the blocks
        g = cases.rough_terrain(21, 73, seed=5, offset=4, relief=2500)
        par = dict(azim_num=12, dist_search=2.0, ray_algorithm="discrete_sampling", hori_acc=0.5)
    elif name == "e_hill":
        g = cases.c2_hill()
        par = dict(azim_num=36, dist_search=10.0)
    else:
        raise KeyError(name)
    return cases.grid_kwargs(g), par, tin


CASES = ("a_guess_constant", "a_binary_search", "a_discrete_sampling", "b_tin", "c_tilted", "d_7_azimuths", "d_1_azimuth",
         "d_13x65", "e_hill")
NO_NAN = ("b_tin", "e_hill")              # the reference has a distance everywhere


def _dist_par(par):
    return {k: v for k, v in par.items() if k in ("dist_search", "hori_acc", "elev_ang_low_lim")}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's horizon of the case and the reference distances of it: computed once, shared, read only."""
    from oracle import oracle as orc
    kw, par, tin = _case(name)
    hori, _ = orc.horizon_gridded(**kw, **par, **tin)
    dist = ref.horizon_distance(**kw, hori=hori, **_dist_par(par), vert_simp=tin.get("vert_simp"),
                                tri_ind_simp=tin.get("tri_ind_simp"))
    share = float(np.isnan(dist).mean())
    print("%s: %.1f %% of the reference distances are NaN" % (name, 100.0 * share))
    assert share <= 0.30, (name, share)
    if name in NO_NAN:
        assert share == 0.0, (name, share)
    hori.setflags(write=False)
    dist.setflags(write=False)
    return hori, dist


def _same(a, b):
    return a.shape == b.shape and np.array_equal(ref.words(a), ref.words(b))


def _planes(a):
    return np.ascontiguousarray(np.moveaxis(a, 2, 0))


@pytest.mark.parametrize("name", CASES)
def test_stand_alone_call_in_both_layouts(hip, orc, name):
    kw, par, tin = _case(name)
    hori, dist = _reference(name)
    got = hip.horizon.horizon_distance(**kw, hori=hori, **_dist_par(par), **tin)
    assert got.dtype == np.float32 and _same(got, dist)
    st = hip.horizon.last_stats
    assert st["num_rays"] == hori.size and st["num_cells"] == hori.shape[0] * hori.shape[1] and st["t_kernel_s"] > 0.0
    got = hip.horizon.horizon_distance(**kw, hori=_planes(hori), **_dist_par(par), **tin, layout="azim_major")
    assert _same(got, _planes(dist))


@pytest.mark.parametrize("name", CASES)
def test_visiting_order_and_block_shape_do_not_matter(hip, orc, name):
    """The distance is the minimum over all accepted triangles: hz_closest's slot order gives the words of the front-to-back
    order, and flatter blocks of cells those of the 8 x 8 block."""
    from horayzon_amd import _lib
    kw, par, tin = _case(name)
    hori, dist = _reference(name)
    L = _lib.lib()
    try:
        for knob, values in ((b"horidist_traversal", (0, 1)), (b"horidist_block_w", (16, 32, 64, 8))):
            for v in values:
                _lib.check(L.hz_debug_set(knob, v))
                assert _same(hip.horizon.horizon_distance(**kw, hori=hori, **_dist_par(par), **tin), dist), (knob, v)
                got = hip.horizon.horizon_distance(**kw, hori=_planes(hori), **_dist_par(par), **tin, layout="azim_major")
                assert _same(got, _planes(dist)), (knob, v)
    finally:
        _lib.check(L.hz_debug_set(b"horidist_traversal", -1))
        _lib.check(L.hz_debug_set(b"horidist_block_w", -1))


@pytest.mark.parametrize("name", CASES)
def test_from_codes(hip, orc, name):
    """A horizon given as 16-bit codes is the float32 horizon decode(q)."""
    kw, par, tin = _case(name)
    hori, _ = _reference(name)
    q = hip.horizon.quantise(hori)
    want = ref.horizon_distance(**kw, hori=hip.horizon.dequantise(q), **_dist_par(par), vert_simp=tin.get("vert_simp"),
                                tri_ind_simp=tin.get("tri_ind_simp"))
    assert _same(hip.horizon.horizon_distance(**kw, hori=q, **_dist_par(par), **tin), want)
    got = hip.horizon.horizon_distance(**kw, hori=_planes(q), **_dist_par(par), **tin, layout="azim_major")
    assert _same(got, _planes(want))


@pytest.mark.parametrize("name", CASES)
def test_mask_rows_chunks_and_scene(hip, orc, name):
    kw, par, tin = _case(name)
    hori, dist = _reference(name)
    in0, in1, _ = hori.shape
    nan = np.float32(np.nan)
    # a 30 % random mask: masked cells are NaN, the others unchanged
    mask = (np.random.default_rng(11).random((in0, in1)) >= 0.3).astype(np.uint8)
    want = np.where(mask[:, :, None] == 1, dist, nan)
    for layout, lay in (("cell_major", lambda a: a), ("azim_major", _planes)):
        got = hip.horizon.horizon_distance(**kw, hori=lay(hori), **_dist_par(par), **tin, mask=mask, layout=layout)
        assert _same(got, lay(want)), layout
    assert hip.horizon.last_stats["num_cells"] == int(mask.sum())
    # a row slab: NaN outside
    want = np.full(dist.shape, nan, np.float32)
    want[3:9] = dist[3:9]
    for layout, lay in (("cell_major", lambda a: a), ("azim_major", _planes)):
        got = hip.horizon.horizon_distance(**kw, hori=lay(hori), **_dist_par(par), **tin, rows=(3, 9), layout=layout)
        assert _same(got, lay(want)), layout
    # chunk seams
    for layout, lay in (("cell_major", lambda a: a), ("azim_major", _planes)):
        got = hip.horizon.horizon_distance(**kw, hori=lay(hori), **_dist_par(par), **tin, _chunk_rows=5, layout=layout)
        assert _same(got, lay(dist)), layout
    got = hip.horizon.horizon_distance(**kw, hori=hip.horizon.quantise(hori), **_dist_par(par), **tin, _chunk_rows=5)
    assert _same(got, hip.horizon.horizon_distance(**kw, hori=hip.horizon.quantise(hori), **_dist_par(par), **tin))
    # a prebuilt scene
    scene = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"], vert_simp=tin.get("vert_simp"),
                             num_vert_simp=tin.get("num_vert_simp", 0), tri_ind_simp=tin.get("tri_ind_simp"),
                             num_tri_simp=tin.get("num_tri_simp", 0))
    try:
        assert _same(hip.horizon.horizon_distance(**kw, hori=hori, **_dist_par(par), scene=scene), dist)
    finally:
        scene.close()


@pytest.mark.parametrize("name", CASES)
def test_horizon_gridded_with_distances(hip, orc, name):
    """horizon_gridded(hori_dist=True): the horizon and the maps of the call without it, and the distances of the
    stand-alone call on its own float32 horizon -- both layouts, codes, a reduction alongside, two slabs."""
    kw, par, tin = _case(name)
    hori_ref, dist_ref = _reference(name)
    G = hip.horizon.horizon_gridded
    plain, azim0 = G(**kw, **par, **tin)
    hori, dist, azim = G(**kw, **par, **tin, hori_dist=True)
    assert np.array_equal(azim, azim0) and _same(hori, plain)
    assert _same(dist, hip.horizon.horizon_distance(**kw, hori=hori, **_dist_par(par), **tin))
    assert _same(hori, hori_ref) and _same(dist, dist_ref)          # (the GPU's horizon is the oracle's)
    pl, dpl, _ = G(**kw, **par, **tin, hori_dist=True, layout="azim_major")
    assert _same(pl, _planes(hori)) and _same(dpl, _planes(dist))
    assert _same(dpl, hip.horizon.horizon_distance(**kw, hori=pl, **_dist_par(par), **tin, layout="azim_major"))
    # codes: the distances are those of the float32 horizon, not of the codes
    for layout, lay in (("cell_major", lambda a: a), ("azim_major", _planes)):
        q, dq, _ = G(**kw, **par, **tin, hori_dist=True, hori_dtype="uint16", layout=layout)
        assert q.dtype == np.uint16 and np.array_equal(q, lay(hip.horizon.quantise(hori))) and _same(dq, lay(dist)), layout
    # chunk seams and a row slab
    h5, d5, _ = G(**kw, **par, **tin, hori_dist=True, _chunk_rows=5)
    assert _same(h5, hori) and _same(d5, dist)
    hr, dr, _ = G(**kw, **par, **tin, hori_dist=True, rows=(3, 9))
    want_h, want_d = np.full_like(hori, np.nan), np.full_like(dist, np.nan)
    want_h[3:9], want_d[3:9] = hori[3:9], dist[3:9]
    assert _same(hr, want_h) and _same(dr, want_d)
    # two slabs on one device
    hd, dd, _ = G(**kw, **par, **tin, hori_dist=True, devices=[0, 0])
    assert _same(hd, hori) and _same(dd, dist)
    # a mask: hori_fill in the horizon, NaN in the distances
    mask = (np.random.default_rng(12).random(hori.shape[:2]) >= 0.3).astype(np.uint8)
    hm, dm, _ = G(**kw, **par, **tin, hori_dist=True, mask=mask)
    assert _same(hm, G(**kw, **par, **tin, mask=mask)[0])
    assert _same(dm, np.where(mask[:, :, None] == 1, dist, np.float32(np.nan)))
    # a prebuilt scene
    scene = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"], vert_simp=tin.get("vert_simp"),
                             num_vert_simp=tin.get("num_vert_simp", 0), tri_ind_simp=tin.get("tri_ind_simp"),
                             num_tri_simp=tin.get("num_tri_simp", 0))
    try:
        hs, ds, _ = G(**kw, **par, hori_dist=True, scene=scene)
        assert _same(hs, hori) and _same(ds, dist)
    finally:
        scene.close()
    # a reduction alongside (needs two azimuths)
    if par["azim_num"] >= 2:
        tilt = np.zeros(kw["vec_norm"].shape, np.float32)
        tilt[..., 2] = 1.0
        _, _, maps0 = G(**kw, **par, **tin, topo=("svf",), topo_vec_tilt=tilt)
        ht, dt, at, maps = G(**kw, **par, **tin, topo=("svf",), topo_vec_tilt=tilt, hori_dist=True)
        assert _same(ht, hori) and _same(dt, dist) and np.array_equal(at, azim) and _same(maps["svf"], maps0["svf"])
        _, _, svf0 = G(**kw, **par, **tin, svf_vec_tilt=tilt)
        hs, ds, _, svf = G(**kw, **par, **tin, svf_vec_tilt=tilt, hori_dist=True)
        assert _same(hs, hori) and _same(ds, dist) and _same(svf, svf0)
