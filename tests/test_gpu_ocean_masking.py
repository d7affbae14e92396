"""horayzon.ocean_masking on the GPU: coastline_distance and coastline_buffer against the contract of DESIGN.md section 4, bit for
bit.  The yardstick is the NumPy brute force of tests/coast_cases.py (and SciPy's k-d tree where
tests/test_ocean_masking_args.py shows the two to agree bit for bit and the brute force is too slow)."""
import numpy as np
import pytest

from tests import cases
from tests import coast_cases as cc

pytestmark = pytest.mark.gpu


def _call(hip, g, **over):
    a = dict(x_ecef=g["x"], y_ecef=g["y"], z_ecef=g["z"], mask_land=g["land"], pts_ecef=g["pts"])
    a.update(over)
    return hip.ocean_masking.coastline_distance(**a)


def _buffer(hip, g, dist_thr, block_size=11, **over):
    a = dict(x_ecef=g["x"], y_ecef=g["y"], z_ecef=g["z"], mask_land=g["land"], pts_ecef=g["pts"], lat=g["lat"],
             dist_thr=dist_thr, dem_res=g["res"], ellps="sphere", block_size=block_size)
    a.update(over)
    return hip.ocean_masking.coastline_buffer(**a)


@pytest.mark.parametrize("n0,n1,seed", [(150, 200, 7), (230, 131, 11)])
def test_distance_equals_the_brute_force(hip, n0, n1, seed):
    g = cc.coast_grid(n0, n1, seed=seed, hurst=0.5)
    assert 1000 < len(g["pts"]) < 20000
    want = cc.brute_distance(g["x"], g["y"], g["z"], g["land"], g["pts"])
    got = _call(hip, g)
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), g["land"])
    assert cc.same_with_nan(got, want)
    st = hip.ocean_masking.last_stats
    assert st["num_cells"] == int((~g["land"]).sum())
    # non-contiguous inputs: transposed storage, every second column of a wider array, a strided vertex array
    wide = {k: np.repeat(g[k], 2, axis=1) for k in ("x", "y", "z", "land")}
    pts2 = np.repeat(g["pts"], 2, axis=0)
    nc = dict(x_ecef=np.asfortranarray(g["x"]), y_ecef=wide["y"][:, ::2], z_ecef=wide["z"][:, ::2],
              mask_land=wide["land"][:, ::2], pts_ecef=pts2[::2])
    assert not nc["x_ecef"].flags["C_CONTIGUOUS"] and not nc["mask_land"].flags["C_CONTIGUOUS"]
    assert not nc["pts_ecef"].flags["C_CONTIGUOUS"]
    assert cc.same_with_nan(_call(hip, g, **nc), want)
    # the order of the vertices cannot matter
    assert cc.same_with_nan(_call(hip, g, pts_ecef=np.ascontiguousarray(g["pts"][::-1])), want)


def test_degenerate_vertex_sets(hip):
    g = cc.coast_grid(40, 56, seed=3, hurst=0.5)
    w = ~g["land"]

    def check(pts, **over):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        gg = dict(g, **over)
        got = _call(hip, gg, pts_ecef=pts)
        want = cc.brute_distance(gg["x"], gg["y"], gg["z"], gg["land"], pts)
        assert cc.same_with_nan(got, want), (len(pts), over.keys())
        return got

    none = check(np.empty((0, 3)))
    assert np.all(np.isposinf(none[w])) and np.all(np.isnan(none[~w]))
    check(g["pts"][:1])
    check(g["pts"][:2])
    for n in (7, 8, 9, 64, 65):                                  # round the leaf size and the wave size
        check(g["pts"][:n])
    check(np.tile(g["pts"][5], (300, 1)))                        # all vertices identical
    lat = np.linspace(42.0, 44.0, 500)
    check(np.stack(cc.sphere_ecef(np.full(500, 6.01), lat), axis=1))      # on one meridian
    check(np.stack((np.linspace(4.0e6, 5.0e6, 300), np.full(300, 4.5e5), np.full(300, 4.3e6)), axis=1))   # on one line
    i, j = np.argwhere(w)[len(np.argwhere(w)) // 2]
    hit = check(np.vstack((g["pts"], [[g["x"][i, j], g["y"][i, j], g["z"][i, j]]])))
    assert hit[i, j] == 0.0                                      # a vertex that coincides with a cell centre
    all_land = check(g["pts"], land=np.ones_like(g["land"]))
    assert np.all(np.isnan(all_land))
    all_water = check(g["pts"], land=np.zeros_like(g["land"]))
    assert not np.isnan(all_water).any()
    for sl in ((slice(None), slice(3, 4)), (slice(5, 6), slice(None))):           # grids one cell wide / high
        check(g["pts"], **{k: np.ascontiguousarray(g[k][sl]) for k in ("x", "y", "z", "land")})
    far = cc.sphere_ecef(np.array([[100.0, 101.0, 102.0]]), np.array([[-40.0, -40.0, -41.0]]))   # about 10 000 km from every vertex
    got = check(g["pts"], x=far[0], y=far[1], z=far[2], land=np.zeros((1, 3), bool))
    assert np.all(got > 9.0e6)


def test_buffer_equals_brute_force_at_every_threshold(hip):
    g = cc.coast_grid(150, 200, seed=7, hurst=0.5)
    w = ~g["land"]
    dist = cc.brute_distance(g["x"], g["y"], g["z"], g["land"], g["pts"])
    chord = hip.ocean_masking.chord_max(g["lat"], g["res"], "sphere", 11)
    d_max = np.nanmax(dist)
    assert d_max > 2.0 * chord
    for thr, kind in ((2.0 * d_max, "none"), (0.5 * (chord + d_max), "some"), (chord, "some")):
        got = _buffer(hip, g, thr)
        assert got.dtype == np.bool_ and got.shape == dist.shape
        want = np.zeros(dist.shape, bool)
        want[w] = dist[w] > thr
        assert np.array_equal(got, want), thr
        assert {"none": not got.any(), "some": got.any() and not got[w].all()}[kind]
    # all masked: no threshold above chord_max does that with this coast, so block_size = 1 (chord_max = 0) and a tiny threshold
    got = _buffer(hip, g, 1.0e-3, block_size=1)
    assert np.array_equal(got, w)
    # the knife edge: a water cell exactly dist_thr away stays inside, the next smaller threshold puts it outside
    cand = np.argwhere(w & (dist > 1.5 * chord))
    for i, j in cand[:: max(1, len(cand) // 5)][:5]:
        d = dist[i, j]
        inside = _buffer(hip, g, d)
        outside = _buffer(hip, g, np.nextafter(d, 0.0))
        assert not inside[i, j] and outside[i, j]
        for got, thr in ((inside, d), (outside, np.nextafter(d, 0.0))):
            want = np.zeros(dist.shape, bool)
            want[w] = dist[w] > thr
            assert np.array_equal(got, want)
    # an empty vertex set is infinitely far away
    assert np.array_equal(_buffer(hip, g, 1.0e5, pts_ecef=np.empty((0, 3))), w)


def _reference_block_algorithm(g, dist_thr, block_size, chord_max, tree):
    """The reference's coastline_buffer restated (ocean_masking.py:283-345): the centre of every block is queried, blocks whose
    centre is nearer than dist_thr - chord_max are inside, farther than dist_thr + chord_max outside, the cells of the remaining
    blocks (and of the rows / columns past the last centre) are queried one by one; land cells are inside."""
    x, y, z, land = g["x"], g["y"], g["z"], g["land"]
    half = (block_size - 1) // 2
    sl = (slice(half, None, block_size), slice(half, None, block_size))
    shp = x[sl].shape
    d_c = tree.query(np.stack((x[sl].ravel(), y[sl].ravel(), z[sl].ravel()), axis=1), k=1)[0].reshape(shp)
    cls = np.full(shp, -1, np.int32)
    cls[d_c <= dist_thr - chord_max] = 0
    cls[d_c > dist_thr + chord_max] = 1
    out = np.full(x.shape, -1, np.int32)
    rep = np.repeat(np.repeat(cls, block_size, axis=0), block_size, axis=1)[:x.shape[0], :x.shape[1]]
    out[:rep.shape[0], :rep.shape[1]] = rep
    rem = out == -1
    out[rem] = tree.query(np.stack((x[rem], y[rem], z[rem]), axis=1), k=1)[0] > dist_thr
    out[land] = 0
    return out.astype(bool), int(rem.sum())


@pytest.mark.parametrize("block_size", [11, 5])
def test_buffer_equals_the_references_block_algorithm(hip, block_size):
    spatial = pytest.importorskip("scipy.spatial")
    g = cc.coast_grid(157, 203, seed=13, hurst=0.5)              # sides that are multiples of neither 11 nor 5
    assert all(n % b for n in g["land"].shape for b in (11, 5))
    chord = hip.ocean_masking.chord_max(g["lat"], g["res"], "sphere", block_size)
    # the premise of the block algorithm, in NumPy: no cell is farther from its block's centre than chord_max
    half = (block_size - 1) // 2
    worst = 0.0
    n0, n1 = g["land"].shape
    for ci in range(half, n0, block_size):
        for cj in range(half, n1, block_size):
            blk = (slice(ci - half, ci + half + 1), slice(cj - half, cj + half + 1))
            d2 = (g["x"][blk] - g["x"][ci, cj]) ** 2 + (g["y"][blk] - g["y"][ci, cj]) ** 2 + (g["z"][blk] - g["z"][ci, cj]) ** 2
            worst = max(worst, float(np.sqrt(d2.max())))
    assert 0.0 < worst <= chord
    tree = spatial.KDTree(g["pts"])
    thr = 2.0 * chord
    want, queried = _reference_block_algorithm(g, thr, block_size, chord, tree)
    assert 0 < queried < g["land"].size and want.any() and not want[~g["land"]].all()   # all three classes of blocks occur
    assert np.array_equal(_buffer(hip, g, thr, block_size=block_size), want)


def test_band_of_the_full_domain_against_the_kd_tree(hip):
    """A 512-row band of the 3569-column inner domain, P = 108 634 coastline vertices (fractal mask with Hurst exponent 0.3,
    seed 3), about 1.0 million water cells: distance and buffer against SciPy's k-d tree, which
    tests/test_ocean_masking_args.py::test_yardstick_brute_force_equals_the_kd_tree_bit_for_bit licenses as yardstick."""
    spatial = pytest.importorskip("scipy.spatial")
    g = cc.coast_grid(512, 3569, seed=3, hurst=0.3)
    assert 1.0e5 <= len(g["pts"]) <= 1.0e6
    w = ~g["land"]
    want = np.full(g["x"].shape, np.nan)
    want[w] = spatial.KDTree(g["pts"]).query(np.stack((g["x"][w], g["y"][w], g["z"][w]), axis=1), k=1, workers=-1)[0]
    got = _call(hip, g)
    assert cc.same_with_nan(got, want)
    thr = float(np.nanmedian(want))
    assert thr > hip.ocean_masking.chord_max(g["lat"], g["res"], "sphere", 11)
    mask = _buffer(hip, g, thr)
    want_mask = np.zeros(w.shape, bool)
    want_mask[w] = want[w] > thr
    assert np.array_equal(mask, want_mask) and mask.any()


def test_stats(hip):
    g = cc.coast_grid(150, 200, seed=7, hurst=0.5)
    chord = hip.ocean_masking.chord_max(g["lat"], g["res"], "sphere", 11)
    water = int((~g["land"]).sum())
    seen = []
    for thr in (None, 2.0 * chord, 10.0 * chord):
        if thr is None:
            _call(hip, g)
        else:
            _buffer(hip, g, thr)
        st = hip.ocean_masking.last_stats
        assert st["t_bvh_s"] > 0 and st["t_kernel_s"] > 0 and st["t_total_s"] >= st["t_bvh_s"] + st["t_kernel_s"]
        assert st["t_h2d_s"] > 0 and st["t_d2h_s"] > 0
        assert st["num_cells"] == water
        assert st["scratch_bytes"] > 0
        seen.append(st["scratch_bytes"])
    assert seen[1] == seen[2] == seen[0]


def test_device_tensors_in_and_out(hip):
    torch = pytest.importorskip("torch")
    g = cc.coast_grid(150, 200, seed=7, hurst=0.5)
    want = cc.brute_distance(g["x"], g["y"], g["z"], g["land"], g["pts"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(g[k])).cuda() for k in ("x", "y", "z", "land", "pts")}
    got = hip.ocean_masking.coastline_distance(dev["x"], dev["y"], dev["z"], dev["land"], dev["pts"])
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64
    assert cc.same_with_nan(got.cpu().numpy(), want)
    assert hip.ocean_masking.last_stats["t_d2h_s"] < 0.5 * hip.ocean_masking.last_stats["t_total_s"]
    thr = float(np.nanmedian(want))
    mask = hip.ocean_masking.coastline_buffer(dev["x"], dev["y"], dev["z"], dev["land"], dev["pts"], g["lat"], thr, g["res"],
                                              "sphere")
    assert isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.bool
    assert np.array_equal(mask.cpu().numpy(), np.nan_to_num(want, nan=0.0) > thr)
    with pytest.raises(ValueError, match="mixed"):
        hip.ocean_masking.coastline_distance(dev["x"], dev["y"], dev["z"], g["land"], g["pts"])


def test_mask_drops_into_horizon_gridded(hip):
    """dtype and orientation fit: mask = ones; mask[coastline_buffer(...)] = 0 gives hori_fill exactly at the masked cells."""
    h = cases.rough_terrain(40, 44, seed=4, offset=4)
    kw = cases.grid_kwargs(h)
    inner = kw["vec_norm"].shape[:2]
    g = cc.coast_grid(inner[0], inner[1], seed=21, hurst=0.5)
    dist = cc.brute_distance(g["x"], g["y"], g["z"], g["land"], g["pts"])
    thr = float(np.nanmedian(dist))
    outside = _buffer(hip, g, thr, block_size=1)
    assert outside.shape == inner and outside.any() and not outside.all()
    mask = np.ones(inner, np.uint8)
    mask[outside] = 0
    hori = hip.horizon.horizon_gridded(**kw, dist_search=1.0, azim_num=8, mask=mask, hori_fill=-7.0)[0]
    hori = np.asarray(hori)
    filled = np.all(hori == np.float32(-7.0), axis=2)
    assert np.array_equal(filled, outside)
