"""HorizonTerrain on the GPU against the NumPy reference of DESIGN.md section 4 clause 10 (tests/horisun_reference.py), and its
float32 set-up against Terrain's.

Bars: shadow codes and sw_dir_cor are bit-identical to the reference at every (cell, position) whose reference margin
|alpha - h| exceeds 1e-9 rad (>= 1e5 times the float64 rounding of the chain's ~20 operations and libm calls, 1/50 of the
float32 spacing of a horizon angle near 1 rad); inside the margin either terrain decision is accepted, with the value that
belongs to the decision taken; at most 1e-4 of a case's unmasked pairs may lie inside (asserted for every case from the
reference alone in tests/test_horisun_reference.py, and again here)."""
import numpy as np
import pytest

from horayzon_amd import synth
from horayzon_amd.shadow import gridded_azimuths
from tests import horisun_reference as R

pytestmark = pytest.mark.gpu

_REF = {}


def ref_of(name):
    """(case, reference) computed once per session and left unchanged."""
    if name not in _REF:
        c = R.case(name)
        _REF[name] = (c, R.reference(c))
    return _REF[name]


class horisun_chunk:
    """hz_debug_set("horisun_chunk", k) for the block, the default restored afterwards."""

    def __init__(self, k):
        self.k = k

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"horisun_chunk", self.k))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"horisun_chunk", -1))
        return False


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """Bit for bit; NaNs (the fill value) only have to be NaNs on both sides."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan]))


def terrain(hip, c, hori=None):
    t = hip.shadow.HorizonTerrain()
    t.initialise(gridded_azimuths(c["azim_num"]), c["hori"] if hori is None else hori, c["vert_grid"], c["dem_dim_0"],
                 c["dem_dim_1"], c["offset_0"], c["offset_1"], c["vec_tilt"], c["vec_norm"], c["vec_north"],
                 c["surf_enl_fac"], c["mask"], sw_dir_cor_fill=c["fill"], ang_max=c["ang_max"])
    return t


def batch_maps(t, suns, shape):
    sh = np.full((suns.shape[0],) + shape, 77, np.uint8)
    sw = np.full((suns.shape[0],) + shape, 77.0, np.float32)
    t.shadow_batch(suns, sh)
    t.sw_dir_cor_batch(suns, sw)
    return sh, sw


def weights_for(n, seed=7):
    w = np.random.default_rng(seed).uniform(0.05, 3.0, n).astype(np.float32)
    w[::4] = 0.0
    return w


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_matches_the_reference_outside_the_margin(hip, name):
    c, ref = ref_of(name)
    mask, suns = c["mask"], c["suns"]
    S = suns.shape[0]
    t = terrain(hip, c)
    with horisun_chunk(R.CHUNK_TEST):                          # S = 5 runs in two launches
        sh, sw = batch_maps(t, suns, mask.shape)
        w = weights_for(S)
        sum_sw = np.full(mask.shape, 77.0, np.float32)
        sum_lit = np.full(mask.shape, 77.0, np.float32)
        t.accumulate(suns, w, sw_dir_cor_sum=sum_sw, sunlit_sum=sum_lit)
    inside = ref["margin"] <= R.MARGIN
    unmasked_pairs = int((mask == 1).sum()) * S
    flips = int(((sh != ref["code"]) & inside).sum())
    print("%s: %d unmasked pairs, %d inside the margin, %d of them decided the other way, smallest margin %.3g rad"
          % (name, unmasked_pairs, int(inside.sum()), flips, float(ref["margin"].min())))
    assert inside.sum() <= R.CAP * unmasked_pairs
    # outside the margin: bit-identical
    assert np.array_equal(sh[~inside], ref["code"][~inside])
    assert same(sw[~inside], ref["val"][~inside])
    # inside: either decision, and the value of the decision taken
    took_ref = sh == ref["code"]
    assert np.array_equal(sh[inside & ~took_ref], ref["code_alt"][inside & ~took_ref])
    assert same(sw[inside & took_ref], ref["val"][inside & took_ref])
    assert same(sw[inside & ~took_ref], ref["val_alt"][inside & ~took_ref])
    # masked cells
    assert (sh[:, mask != 1] == 3).all() and np.isnan(sw[:, mask != 1]).all()
    # the single-position forms write the batch maps' planes
    one_sh, one_sw = np.empty(mask.shape, np.uint8), np.empty(mask.shape, np.float32)
    t.shadow(suns[S - 1], one_sh)
    t.sw_dir_cor(suns[S - 1], one_sw)
    assert same(one_sh, sh[S - 1]) and same(one_sw, sw[S - 1])
    # accumulate: the clause 9 fold of the GPU's own maps, bit for bit; and the reference's fold where no pair of the cell is inside
    own_sw, own_lit = R.fold(sh, sw, w, mask, c["fill"])
    assert same(sum_sw, own_sw) and same(sum_lit, own_lit)
    ref_sw, ref_lit = R.fold(ref["code"], ref["val"], w, mask, c["fill"])
    clean = ~inside.any(axis=0)
    assert same(sum_sw[clean], ref_sw[clean]) and same(sum_lit[clean], ref_lit[clean])
    assert np.isnan(sum_sw[mask != 1]).all() and np.isnan(sum_lit[mask != 1]).all()


def test_chunks_outputs_in_one_call_and_unit_weights(hip):
    c, _ = ref_of("inner_A7_random")
    mask, suns = c["mask"], c["suns"]
    S = suns.shape[0]
    t = terrain(hip, c)
    sh, sw = batch_maps(t, suns, mask.shape)                   # default chunk: one launch
    w = weights_for(S, seed=3)
    base_sw, base_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
    t.accumulate(suns, w, sw_dir_cor_sum=base_sw, sunlit_sum=base_lit)
    for k in (1, 2, 4, 5):
        with horisun_chunk(k):
            sh_k, sw_k = batch_maps(t, suns, mask.shape)
            # all four outputs from one call
            a_sh, a_sw = np.empty_like(sh), np.empty_like(sw)
            a_sum, a_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
            t.accumulate(suns, w, sw_dir_cor_sum=a_sum, sunlit_sum=a_lit, shadow_buffers=a_sh, sw_dir_cor_buffers=a_sw)
            # one sum alone
            only_sw, only_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
            t.accumulate(suns, w, sw_dir_cor_sum=only_sw)
            t.accumulate(suns, w, sunlit_sum=only_lit)
        assert same(sh_k, sh) and same(sw_k, sw), k
        assert same(a_sh, sh) and same(a_sw, sw) and same(a_sum, base_sw) and same(a_lit, base_lit), k
        assert same(only_sw, base_sw) and same(only_lit, base_lit), k
    # weights=None equals ones
    none_sw, none_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
    ones_sw, ones_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
    t.accumulate(suns, None, sw_dir_cor_sum=none_sw, sunlit_sum=none_lit)
    t.accumulate(suns, np.ones(S, np.float32), sw_dir_cor_sum=ones_sw, sunlit_sum=ones_lit)
    assert same(none_sw, ones_sw) and same(none_lit, ones_lit)
    assert same(none_lit, R.fold(sh, sw, None, mask, c["fill"])[1])


def test_scratch_does_not_grow_with_the_positions(hip):
    c, _ = ref_of("inner_A2_random")
    t = terrain(hip, c)
    rng = np.random.default_rng(5)
    suns = (1.5e11 * R.unit(rng.standard_normal((400, 3)))).astype(np.float32)
    out = np.empty(c["mask"].shape, np.float32)
    lit = np.empty(c["mask"].shape, np.float32)
    t.accumulate(suns[:50].copy(), None, sw_dir_cor_sum=out, sunlit_sum=lit)        # 50 > the default chunk of 48
    st_few = dict(t.last_stats)
    t.accumulate(suns, None, sw_dir_cor_sum=out, sunlit_sum=lit)
    st_many = dict(t.last_stats)
    assert st_few["scratch_bytes"] > 0 and st_few["t_kernel_s"] > 0
    assert st_few["scratch_bytes"] == st_many["scratch_bytes"]


def test_device_horizon_and_device_buffers_give_the_same_bytes(hip):
    torch = pytest.importorskip("torch")
    c, _ = ref_of("inner_A360_planar")
    mask, suns = c["mask"], c["suns"]
    S = suns.shape[0]
    w = weights_for(S, seed=11)
    t = terrain(hip, c)
    sh, sw = batch_maps(t, suns, mask.shape)
    sum_sw, sum_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
    t.accumulate(suns, w, sw_dir_cor_sum=sum_sw, sunlit_sum=sum_lit)
    dev = "cuda:%d" % t.device
    d_hori = torch.from_numpy(c["hori"]).to(dev)
    torch.cuda.synchronize()
    td = terrain(hip, c, hori=d_hori)
    assert td._hori is d_hori                                  # borrowed: the object holds a reference
    sh_d, sw_d = batch_maps(td, suns, mask.shape)
    assert same(sh_d, sh) and same(sw_d, sw)
    # outputs, positions and weights in HBM
    o_sh = torch.full((S,) + mask.shape, 9, dtype=torch.uint8, device=dev)
    o_sw = torch.full((S,) + mask.shape, 9.0, dtype=torch.float32, device=dev)
    o_sum = torch.full(mask.shape, 9.0, dtype=torch.float32, device=dev)
    o_lit = torch.full(mask.shape, 9.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    td.shadow_batch(suns, o_sh)
    td.sw_dir_cor_batch(suns, o_sw)
    td.accumulate(torch.from_numpy(suns).to(dev), torch.from_numpy(w).to(dev), sw_dir_cor_sum=o_sum, sunlit_sum=o_lit)
    torch.cuda.synchronize()
    assert same(o_sh.cpu().numpy(), sh) and same(o_sw.cpu().numpy(), sw)
    assert same(o_sum.cpu().numpy(), sum_sw) and same(o_lit.cpu().numpy(), sum_lit)
    # several launches, each input from its own side: positions in HBM with host weights, and the other way round
    d_sun, d_w = torch.from_numpy(suns).to(dev), torch.from_numpy(w).to(dev)
    torch.cuda.synchronize()
    for pos, wts in ((d_sun, w), (suns, d_w)):
        a_sh, a_sw = np.full_like(sh, 9), np.full_like(sw, 9.0)
        a_sum, a_lit = np.full(mask.shape, 9.0, np.float32), np.full(mask.shape, 9.0, np.float32)
        with horisun_chunk(2):
            td.accumulate(pos, wts, sw_dir_cor_sum=a_sum, sunlit_sum=a_lit, shadow_buffers=a_sh, sw_dir_cor_buffers=a_sw)
        assert same(a_sh, sh) and same(a_sw, sw) and same(a_sum, sum_sw) and same(a_lit, sum_lit)


def test_setup_is_terrains_bit_for_bit(hip):
    """A flat DEM, where no ray hits anything, under a horizon of -1 rad, which shades nothing: what is left is the float32
    set-up -- origin, sun direction, the two dot products, self-shading, ang_max, the sw_dir_cor formula -- and it must be
    Terrain's (refrac_cor=False) bit for bit.  Tilts up to 80 degrees and suns from just above the plane (a sun below it would send
    Terrain's ray into the ground) to the zenith exercise both tests."""
    n, off = 40, 3
    rng = np.random.default_rng(21)
    x = (np.arange(n) * 25.0).astype(np.float32)
    y = ((n - 1 - np.arange(n)) * 25.0).astype(np.float32)
    xx, yy = np.meshgrid(x, y)
    vert_grid = synth.pack_vertices(xx, yy, np.full((n, n), 250.0, np.float32))
    n0 = n1 = n - 2 * off
    vec_norm, vec_north = synth.planar_frames(n0, n1)
    ang = np.deg2rad(80.0) * rng.random((n0, n1))
    dirn = rng.uniform(0.0, 2.0 * np.pi, (n0, n1))
    vec_tilt = np.stack([np.sin(ang) * np.cos(dirn), np.sin(ang) * np.sin(dirn), np.cos(ang)], axis=2).astype(np.float32)
    enl = rng.uniform(1.0, 2.0, (n0, n1)).astype(np.float32)
    mask = (rng.random((n0, n1)) > 0.1).astype(np.uint8)
    elev = np.full((n0, n1), 250.0, np.float32)
    az = rng.uniform(0.0, 2.0 * np.pi, 12)
    el = np.deg2rad(np.array([0.05, 0.2, 0.6, 0.9, 1.1, 3.0, 10.0, 25.0, 45.0, 70.0, 89.0, 90.0]))
    suns = (1.5e11 * np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)).astype(np.float32)
    for ang_max in (89.0, 85.0):
        tr = hip.shadow.Terrain()
        tr.initialise(vert_grid, n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-3.0, ang_max=ang_max)
        th = hip.shadow.HorizonTerrain()
        th.initialise(gridded_azimuths(16), np.full((n0, n1, 16), -1.0, np.float32), vert_grid, n, n, off, off,
                      vec_tilt, vec_norm, vec_north, enl, mask, sw_dir_cor_fill=-3.0, ang_max=ang_max)
        r_sh, r_sw = batch_maps(tr, suns, mask.shape)
        h_sh, h_sw = batch_maps(th, suns, mask.shape)
        assert not (r_sh == 2).any() and (r_sh == 0).any() and (r_sh == 1).any() and (r_sh == 3).any()
        assert ((r_sh == 0) & (r_sw == 0)).any()                   # lit for shadow(), outside ang_max for sw_dir_cor()
        assert same(h_sh, r_sh) and same(h_sw, r_sw)
        w = weights_for(12, seed=2)
        outs = []
        for t in (tr, th):
            a, b = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
            t.accumulate(suns, w, sw_dir_cor_sum=a, sunlit_sum=b)
            outs.append((a, b))
        assert same(outs[1][0], outs[0][0]) and same(outs[1][1], outs[0][1])
