"""HorizonTerrain with atmospheric refraction on the GPU (clause 13) against the NumPy reference
(tests/horisun_refrac_reference.py), its float32 set-up against Terrain(refrac_cor=True), the block means of
sw_dir_cor_coarse on both routes, and the switch itself -- for both horizon layouts.

Bars: clause 10's (tests/test_gpu_horisun.py).  Shadow codes and sw_dir_cor are bit-identical to the reference at every
(cell, position) whose reference margin |alpha - h| exceeds 1e-9 rad; inside the margin either terrain decision is accepted,
with the value that belongs to the decision taken; at most 1e-4 of a case's unmasked pairs may lie inside.  The float32 part
of the chain -- the refraction included -- is exact on both sides, so the margin covers the float64 look-up alone.
tests/test_horisun_refrac_reference.py shows from the reference alone that refraction changes more than 1 in 100 codes of the
low-sun cases: a kernel or route that takes the switch and does not apply it fails here."""
import numpy as np
import pytest

from horayzon_amd import synth
from horayzon_amd.shadow import gridded_azimuths
from tests import horisun_coarse_cases as K
from tests import horisun_reference as R
from tests import horisun_refrac_reference as RR

pytestmark = pytest.mark.gpu

same = K.same


class debug_set:
    """hz_debug_set(key, value) for the block, the default restored afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, -1))
        return False


def chunk(k):
    return debug_set(b"horisun_chunk", k)


def route(r):
    return debug_set(b"horisun_coarse_route", r)


def make(hip, c, planes=False, refrac=True):
    t = hip.shadow.HorizonTerrain()
    hori = np.ascontiguousarray(c["hori"].transpose(2, 0, 1)) if planes else c["hori"]
    (t.initialise_azim_major if planes else t.initialise)(
        gridded_azimuths(c["azim_num"]), hori, c["vert_grid"], c["dem_dim_0"], c["dem_dim_1"], c["offset_0"], c["offset_1"],
        c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], c["mask"], sw_dir_cor_fill=c["fill"],
        ang_max=c["ang_max"])
    assert t.refrac_cor is False
    if refrac:
        t.refraction(c["elevation"])
        assert t.refrac_cor is True
    return t


_OBJ = {}


def obj(hip, name, planes=False):
    """The refracting HorizonTerrain of (case, layout): made once per session."""
    if (name, planes) not in _OBJ:
        _OBJ[(name, planes)] = make(hip, RR.case(name)[0], planes)
    return _OBJ[(name, planes)]


def batch_maps(t, suns):
    sh = np.full((suns.shape[0],) + t._shape, 77, np.uint8)
    sw = np.full((suns.shape[0],) + t._shape, 77.0, np.float32)
    t.shadow_batch(suns, sh)
    t.sw_dir_cor_batch(suns, sw)
    return sh, sw


_MAPS = {}


def maps(hip, name):
    """The cell-major object's batch maps at the test chunk: computed once, never written again."""
    if name not in _MAPS:
        with chunk(RR.CHUNK_TEST):
            sh, sw = batch_maps(obj(hip, name), RR.case(name)[0]["suns"])
        sh.setflags(write=False)
        sw.setflags(write=False)
        _MAPS[name] = (sh, sw)
    return _MAPS[name]


def weights_for(n, seed=7):
    w = np.random.default_rng(seed).uniform(0.05, 3.0, n).astype(np.float32)
    w[::4] = 0.0
    return w


def sums(t, suns, w):
    a, b = np.full(t._shape, 77.0, np.float32), np.full(t._shape, 77.0, np.float32)
    t.accumulate(suns, w, sw_dir_cor_sum=a, sunlit_sum=b)
    return a, b


@pytest.mark.parametrize("planes", (False, True))
@pytest.mark.parametrize("name", RR.NAMES)
def test_matches_the_reference_outside_the_margin(hip, name, planes):
    c, ref = RR.case(name)
    mask, suns = c["mask"], c["suns"]
    S = suns.shape[0]
    t = obj(hip, name, planes)
    w = weights_for(S)
    with chunk(RR.CHUNK_TEST):                                  # S = 6 or 7 runs in two or three launches
        sh, sw = batch_maps(t, suns)
        sum_sw, sum_lit = sums(t, suns, w)
    inside = ref["margin"] <= R.MARGIN
    unmasked_pairs = int((mask == 1).sum()) * S
    flips = int(((sh != ref["code"]) & inside).sum())
    print("%s planes=%d: %d unmasked pairs, %d inside the margin, %d of them decided the other way, smallest margin %.3g rad"
          % (name, planes, unmasked_pairs, int(inside.sum()), flips, float(ref["margin"].min())))
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
    # the planes words are the cell-major words
    base_sh, base_sw = maps(hip, name)
    assert same(sh, base_sh) and same(sw, base_sw)


@pytest.mark.parametrize("planes", (False, True))
def test_position_chunks_give_the_same_words(hip, planes):
    name = "low_A360_planar"
    c, _ = RR.case(name)
    suns = c["suns"]
    t = obj(hip, name, planes)
    w = weights_for(suns.shape[0], seed=3)
    sh, sw = batch_maps(t, suns)                                # the default chunk: one launch
    base = sums(t, suns, w)
    assert same(sh, maps(hip, name)[0]) and same(sw, maps(hip, name)[1])
    for k in (1, 3):
        with chunk(k):
            sh_k, sw_k = batch_maps(t, suns)
            sums_k = sums(t, suns, w)
            a_sh, a_sw = np.empty_like(sh), np.empty_like(sw)
            a_sum, a_lit = np.empty(t._shape, np.float32), np.empty(t._shape, np.float32)
            t.accumulate(suns, w, sw_dir_cor_sum=a_sum, sunlit_sum=a_lit, shadow_buffers=a_sh, sw_dir_cor_buffers=a_sw)
        assert same(sh_k, sh) and same(sw_k, sw), k
        assert same(sums_k[0], base[0]) and same(sums_k[1], base[1]), k
        assert same(a_sh, sh) and same(a_sw, sw) and same(a_sum, base[0]) and same(a_lit, base[1]), k


def test_setup_is_terrains_bit_for_bit(hip):
    """The flat DEM of tests/test_gpu_horisun.py::test_setup_is_terrains_bit_for_bit, where no ray hits anything, under a
    horizon of -1 rad, which shades nothing, with elevations from 0 to 2000 m: what is left is the float32 set-up with the
    refraction, and it must be Terrain's (refrac_cor=True) word for word.  Suns from -0.2 degrees true elevation -- the refraction
    there is at least 0.4 degrees, so every refracted sun is above the plane and Terrain's ray leaves the ground -- to the zenith."""
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
    elev = rng.uniform(0.0, 2000.0, (n0, n1)).astype(np.float32)
    az = rng.uniform(0.0, 2.0 * np.pi, 12)
    el = np.deg2rad(np.array([-0.2, -0.1, 0.05, 0.2, 0.6, 1.1, 3.0, 10.0, 25.0, 45.0, 89.0, 90.0]))
    suns = (1.5e11 * np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)).astype(np.float32)
    w = weights_for(12, seed=2)
    for ang_max in (89.0, 85.0):
        tr = hip.shadow.Terrain()
        tr.initialise(vert_grid, n, n, off, off, vec_tilt, vec_norm, enl, elev, mask, sw_dir_cor_fill=-3.0, ang_max=ang_max,
                      refrac_cor=True)
        r_sh = np.full((12,) + mask.shape, 77, np.uint8)
        r_sw = np.full((12,) + mask.shape, 77.0, np.float32)
        tr.shadow_batch(suns, r_sh)
        tr.sw_dir_cor_batch(suns, r_sw)
        assert not (r_sh == 2).any() and (r_sh == 0).any() and (r_sh == 1).any() and (r_sh == 3).any()
        assert (r_sh[0] == 0).any()                                # lit under the -0.2 degree sun: the refraction acted
        r_sum, r_lit = np.empty(mask.shape, np.float32), np.empty(mask.shape, np.float32)
        tr.accumulate(suns, w, sw_dir_cor_sum=r_sum, sunlit_sum=r_lit)
        for planes in (False, True):
            th = hip.shadow.HorizonTerrain()
            hori = np.full((16, n0, n1) if planes else (n0, n1, 16), -1.0, np.float32)
            (th.initialise_azim_major if planes else th.initialise)(
                gridded_azimuths(16), hori, vert_grid, n, n, off, off, vec_tilt, vec_norm, vec_north, enl, mask,
                sw_dir_cor_fill=-3.0, ang_max=ang_max)
            th.refraction(elev)
            h_sh, h_sw = batch_maps(th, suns)
            assert same(h_sh, r_sh) and same(h_sw, r_sw), (ang_max, planes)
            h_sum, h_lit = sums(th, suns, w)
            assert same(h_sum, r_sum) and same(h_lit, r_lit), (ang_max, planes)


def coarse(t, suns, P, sw=True, lit=True, r=0):
    """One call on route r: 0 the fused kernel, 1 the two-pass route."""
    P0, P1 = K.pair(P)
    shape = (suns.shape[0], t._shape[0] // P0, t._shape[1] // P1)
    f_cor = np.full(shape, 123.0, np.float32) if sw else None
    frac = np.full(shape, 123.0, np.float32) if lit else None
    with route(r):
        t.sw_dir_cor_coarse(suns, P, f_cor=f_cor, sunlit_frac=frac)
    return f_cor, frac


@pytest.mark.parametrize("planes", (False, True))
@pytest.mark.parametrize("r", (0, 1))
@pytest.mark.parametrize("name", RR.COARSE)
def test_coarse_is_the_block_mean_of_the_refracted_maps(hip, name, r, planes):
    c, ref = RR.case(name)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    t = obj(hip, name, planes)
    sh, sw = maps(hip, name)
    inside = ref["margin"] <= R.MARGIN
    with chunk(RR.CHUNK_TEST):
        for P in RR.PIXELS[name]:
            own_f, own_l = K.block_means(sw, sh, mask, P, fill)
            ref_f, ref_l = K.block_means(ref["val"], ref["code"], mask, P, fill)
            held = ~K.block_any(inside, P)                          # blocks without a pair inside the margin
            assert (~held).sum() <= R.CAP * held.size, P
            f_cor, frac = coarse(t, suns, P, r=r)
            f1, none_l = coarse(t, suns, P, lit=False, r=r)
            none_f, l1 = coarse(t, suns, P, sw=False, r=r)
            assert none_l is None and none_f is None
            for f, l in ((f_cor, frac), (f1, l1)):
                assert same(f, own_f) and same(l, own_l), P
                assert same(f[held], ref_f[held]) and same(l[held], ref_l[held]), P


@pytest.mark.parametrize("planes", (False, True))
def test_switching(hip, planes):
    name = "coarse_low_A360_planar"
    c, _ = RR.case(name)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    w = weights_for(suns.shape[0], seed=5)
    P = (6, 20)

    def answers(t):
        out = list(batch_maps(t, suns)) + list(sums(t, suns, w))
        for r in (0, 1):
            out += list(coarse(t, suns, P, r=r))
        return out

    def equal(a, b):
        return all(same(x, y) for x, y in zip(a, b))

    plain = answers(make(hip, c, planes, refrac=False))          # an object that never had it
    bent = [maps(hip, name)[0], maps(hip, name)[1]]
    assert not same(plain[0], bent[0]) and not same(plain[1], bent[1])
    t = make(hip, c, planes)
    on = answers(t)
    assert equal(on[:2], bent)
    t.refraction(None)
    assert t.refrac_cor is False and equal(answers(t), plain)
    # twice with different elevations: the second counts
    other = np.ascontiguousarray(c["elevation"][::-1, ::-1]) + np.float32(700.0)
    t.refraction(other)
    t.refraction(c["elevation"])
    assert t.refrac_cor is True and equal(answers(t), on)
    t.refraction(other)
    fac = RR.refrac_factor(other)
    ref = RR.lookup_refrac(suns, c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], mask, fill,
                           c["ang_max"], fac)
    got = answers(t)
    held = ref["margin"] > R.MARGIN
    assert np.array_equal(got[0][held], ref["code"][held]) and same(got[1][held], ref["val"][held])
    assert not same(got[0], on[0])
    # initialise again switches it off, as a fresh object would be
    hori = np.ascontiguousarray(c["hori"].transpose(2, 0, 1)) if planes else c["hori"]
    (t.initialise_azim_major if planes else t.initialise)(
        gridded_azimuths(c["azim_num"]), hori, c["vert_grid"], c["dem_dim_0"], c["dem_dim_1"], c["offset_0"], c["offset_1"],
        c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], mask, sw_dir_cor_fill=fill, ang_max=c["ang_max"])
    assert t.refrac_cor is False and equal(answers(t), plain)
