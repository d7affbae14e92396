"""HorizonTerrain.sw_dir_cor_coarse on the GPU (clause 12): per sun position, the block means of
sw_dir_cor and of the sunlit flag from a stored horizon.

Bar: bit-identical to the block-mean fold (tests/horisun_coarse_cases.py: a sequential float64 add per block in row-major
order) of the NumPy reference's per-position maps, for every block that holds no (cell, position) pair inside the reference's
margin; at most R.CAP of a table's blocks may be excluded so.  tests/test_horisun_coarse_reference.py shows from the reference
alone that the cases exclude nothing.  And bit-identical, without exclusion, to the fold of the object's own batch maps, across
the two horizon layouts, the two routes and every tile and chunk knob."""
import numpy as np
import pytest

from horayzon_amd.shadow import gridded_azimuths
from tests import horisun_coarse_cases as K
from tests import horisun_reference as R

pytestmark = pytest.mark.gpu


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


def route(r):
    return debug_set(b"horisun_coarse_route", r)


def tile(cells):
    return debug_set(b"horisun_coarse_tile", cells)


def chunk(k):
    return debug_set(b"horisun_chunk", k)


def make(hip, c, planes=False):
    t = hip.shadow.HorizonTerrain()
    hori = np.ascontiguousarray(c["hori"].transpose(2, 0, 1)) if planes else c["hori"]
    (t.initialise_azim_major if planes else t.initialise)(
        gridded_azimuths(c["azim_num"]), hori, c["vert_grid"], c["dem_dim_0"], c["dem_dim_1"], c["offset_0"], c["offset_1"],
        c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], c["mask"], sw_dir_cor_fill=c["fill"],
        ang_max=c["ang_max"])
    return t


_OBJ = {}


def obj(hip, name, planes=False):
    """The HorizonTerrain of (case, layout): made once per session."""
    if (name, planes) not in _OBJ:
        _OBJ[(name, planes)] = make(hip, K.case(name)[0], planes)
    return _OBJ[(name, planes)]


_FUSED = {}


def fused(hip, name, P):
    """Both tables of (case, P) from the fused kernel, cell-major: computed once, never written again."""
    if (name, P) not in _FUSED:
        f, l, _ = coarse(obj(hip, name), K.case(name)[0]["suns"], P)
        f.setflags(write=False)
        l.setflags(write=False)
        _FUSED[(name, P)] = (f, l)
    return _FUSED[(name, P)]


def coarse(t, suns, P, sw=True, lit=True, prefill=123.0, r=0):
    """One call on route r: 0 the fused kernel, 1 the two-pass route, -1 the layout's default."""
    P0, P1 = K.pair(P)
    shape = (suns.shape[0], t._shape[0] // P0, t._shape[1] // P1)
    f_cor = np.full(shape, prefill, np.float32) if sw else None
    frac = np.full(shape, prefill, np.float32) if lit else None
    with route(r):
        t.sw_dir_cor_coarse(suns, P, f_cor=f_cor, sunlit_frac=frac)
    return f_cor, frac, dict(t.last_stats)


def batch_maps(t, suns):
    sh = np.full((suns.shape[0],) + t._shape, 77, np.uint8)
    sw = np.full((suns.shape[0],) + t._shape, 77.0, np.float32)
    t.shadow_batch(suns, sh)
    t.sw_dir_cor_batch(suns, sw)
    return sh, sw


@pytest.mark.parametrize("name", K.NAMES)
def test_matches_the_reference(hip, name):
    """Fused route, cell-major, both outputs and each alone, against the fold of the NumPy reference's maps."""
    c, ref = K.case(name)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    t = obj(hip, name)
    inside = ref["margin"] <= R.MARGIN
    for P in K.PIXELS[name]:
        ref_f, ref_l = K.block_means(ref["val"], ref["code"], mask, P, fill)
        held = ~K.block_any(inside, P)                              # blocks without a pair inside the margin
        print("%s P %s: %d of %d blocks excluded" % (name, P, int((~held).sum()), held.size))
        assert (~held).sum() <= R.CAP * held.size, P
        n = np.broadcast_to(K.block_counts(mask, P), ref_f.shape)
        f_cor, frac = fused(hip, name, P)
        assert K.same(f_cor[held], ref_f[held]) and K.same(frac[held], ref_l[held]), P
        assert (f_cor[n > 0] > 0).any(), P
        if (n == 0).any():
            assert K.is_fill(f_cor[n == 0], fill) and K.is_fill(frac[n == 0], fill), P
        # one output alone: the same table
        f1, none_l, _ = coarse(t, suns, P, lit=False)
        none_f, l1, _ = coarse(t, suns, P, sw=False)
        assert none_l is None and none_f is None
        assert K.same(f1, f_cor) and K.same(l1, frac), P
    assert any((K.block_counts(mask, P) == 0).any() for P in K.PIXELS[name])


@pytest.mark.parametrize("name", K.NAMES)
def test_matches_the_fold_of_its_own_maps(hip, name):
    c, _ = K.case(name)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    sh, sw = batch_maps(obj(hip, name), suns)
    for P in K.PIXELS[name]:
        own_f, own_l = K.block_means(sw, sh, mask, P, fill)
        f_cor, frac = fused(hip, name, P)
        assert K.same(f_cor, own_f) and K.same(frac, own_l), P


@pytest.mark.parametrize("name", K.NAMES)
def test_one_cell_per_coarse_cell_is_the_batch_map(hip, name):
    c, _ = K.case(name)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    sh, sw = batch_maps(obj(hip, name), suns)
    f_cor, frac = fused(hip, name, 1)
    on = np.broadcast_to(mask == 1, f_cor.shape)
    assert f_cor.shape == sw.shape
    assert np.array_equal(f_cor[on].view(np.uint32), sw[on].view(np.uint32))
    assert set(np.unique(frac[on])) <= {0.0, 1.0}
    assert np.array_equal(frac[on] == 1.0, sh[on] == 0)
    assert K.is_fill(f_cor[~on], fill) and K.is_fill(frac[~on], fill)


@pytest.mark.parametrize("name", K.NAMES)
def test_layouts_give_the_same_words(hip, name):
    c, _ = K.case(name)
    tp = obj(hip, name, planes=True)
    for P in K.PIXELS[name]:
        f_cor, frac = fused(hip, name, P)
        pf, pl, _ = coarse(tp, c["suns"], P)
        assert K.same(pf, f_cor) and K.same(pl, frac), P
        p1, _, _ = coarse(tp, c["suns"], P, lit=False)
        _, l1, _ = coarse(tp, c["suns"], P, sw=False)
        assert K.same(p1, f_cor) and K.same(l1, frac), P


@pytest.mark.parametrize("planes", (False, True))
@pytest.mark.parametrize("name", K.NAMES)
def test_two_pass_route_gives_the_same_words(hip, name, planes):
    c, _ = K.case(name)
    t = obj(hip, name, planes)
    for P in K.PIXELS[name]:
        f_cor, frac = fused(hip, name, P)
        rf, rl, _ = coarse(t, c["suns"], P, r=1)
        r1, _, _ = coarse(t, c["suns"], P, lit=False, r=1)
        _, l1, _ = coarse(t, c["suns"], P, sw=False, r=1)
        assert K.same(rf, f_cor) and K.same(rl, frac) and K.same(r1, f_cor) and K.same(l1, frac), P
        df, dl, _ = coarse(t, c["suns"], P, r=-1)                   # the layout's default route
        assert K.same(df, f_cor) and K.same(dl, frac), P


@pytest.mark.parametrize("cells", (256, 64, 7))
def test_tile_of_the_fused_kernel_changes_nothing(hip, cells):
    """Small LDS tiles: several strips per coarse row, several tiles per block, and blocks wider than the tile (two-pass)."""
    for name in K.NAMES:
        c, _ = K.case(name)
        for planes in (False, True):
            t = obj(hip, name, planes)
            for P in K.PIXELS[name]:
                f_cor, frac = fused(hip, name, P)
                with tile(cells):
                    tf, tl, _ = coarse(t, c["suns"], P)
                    t1, _, _ = coarse(t, c["suns"], P, lit=False)
                    _, l1, _ = coarse(t, c["suns"], P, sw=False)
                assert K.same(tf, f_cor) and K.same(tl, frac) and K.same(t1, f_cor) and K.same(l1, frac), (name, planes, P)


@pytest.mark.parametrize("k", (1, 2, 3, 7))
def test_chunk_size_does_not_change_the_tables(hip, k):
    """S = 7 with chunk 3: the last chunk is short; chunks of 2 and 3 with more than one position per pass: a pass is short."""
    for name in ("A360", "A7"):
        c, _ = K.case(name)
        assert c["suns"].shape[0] == 7
        for planes in (False, True):
            t = obj(hip, name, planes)
            for P in K.PIXELS[name]:
                f_cor, frac = fused(hip, name, P)
                with chunk(k):
                    kf, kl, _ = coarse(t, c["suns"], P)
                    k1, _, _ = coarse(t, c["suns"], P, lit=False)
                    rf, rl, _ = coarse(t, c["suns"], P, r=1)
                assert K.same(kf, f_cor) and K.same(kl, frac) and K.same(k1, f_cor), (name, planes, P, k)
                assert K.same(rf, f_cor) and K.same(rl, frac), (name, planes, P, k)


def test_scratch_does_not_grow_with_the_positions(hip):
    c, _ = K.case("A360")
    t, suns = obj(hip, "A360"), c["suns"]
    with chunk(3):
        _, _, st3 = coarse(t, suns[:3].copy(), 4)
        _, _, st7 = coarse(t, suns, 4)
        _, _, rt3 = coarse(t, suns[:3].copy(), 4, r=1)
        _, _, rt7 = coarse(t, suns, 4, r=1)
    assert st3["scratch_bytes"] > 0 and st7["t_kernel_s"] > 0 and st7["num_cells"] == c["mask"].size
    assert st3["scratch_bytes"] == st7["scratch_bytes"]
    assert rt3["scratch_bytes"] == rt7["scratch_bytes"]
    assert rt7["scratch_bytes"] >= st7["scratch_bytes"] + 3 * 5 * c["mask"].size     # three positions of maps


@pytest.mark.parametrize("r", (0, 1))
def test_device_buffers_give_the_same_tables(hip, r):
    ref = fused(hip, "A360", (6, 20))
    with route(r):
        _device_buffers(hip, (6, 20), *ref)


def _device_buffers(hip, P, ref_f, ref_l):
    torch = pytest.importorskip("torch")
    c, _ = K.case("A360")
    suns = c["suns"]
    for planes in (False, True):
        t = obj(hip, "A360", planes)
        dev = "cuda:%d" % t.device
        d_sun = torch.from_numpy(suns.copy()).to(dev)
        d_f = torch.full(ref_f.shape, 7.0, dtype=torch.float32, device=dev)
        d_l = torch.full(ref_f.shape, 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t.sw_dir_cor_coarse(d_sun, P, f_cor=d_f, sunlit_frac=d_l)
        torch.cuda.synchronize()
        assert K.same(d_f.cpu().numpy(), ref_f) and K.same(d_l.cpu().numpy(), ref_l)
        # host positions into HBM outputs, and device positions into NumPy outputs
        d_f.fill_(7.0)
        torch.cuda.synchronize()
        t.sw_dir_cor_coarse(suns, P, f_cor=d_f)
        torch.cuda.synchronize()
        assert K.same(d_f.cpu().numpy(), ref_f)
        out = np.empty(ref_l.shape, np.float32)
        t.sw_dir_cor_coarse(d_sun, P, sunlit_frac=out)
        assert K.same(out, ref_l)
        with pytest.raises(ValueError, match="device"):
            t.sw_dir_cor_coarse(suns, P, f_cor=torch.zeros(ref_f.shape, dtype=torch.float32))
        with pytest.raises(ValueError, match="device"):
            t.sw_dir_cor_coarse(torch.from_numpy(suns.copy()), P, f_cor=d_f)


def test_outputs_are_not_read(hip):
    c, _ = K.case("A7")                                             # fill -9.0
    for planes in (False, True):
        t = obj(hip, "A7", planes)
        for r in (0, 1):
            a_f, a_l, _ = coarse(t, c["suns"], 4, prefill=123.0, r=r)
            b_f, b_l, _ = coarse(t, c["suns"], 4, prefill=np.nan, r=r)
            assert K.same(a_f, b_f) and K.same(a_l, b_l)
            assert not np.isnan(a_f).any() and (a_f != 123.0).all() and (a_l != 123.0).all()   # every element is written


def test_calls_leave_no_state(hip):
    c, _ = K.case("A7")
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    t = make(hip, c)
    sh, sw = batch_maps(t, suns)
    f_cor, frac, _ = coarse(t, suns, 4)
    own_f, own_l = K.block_means(sw, sh, mask, 4, fill)
    assert K.same(f_cor, own_f) and K.same(frac, own_l)
    acc_sw = np.full(mask.shape, 123.0, np.float32)
    acc_lit = np.full(mask.shape, 123.0, np.float32)
    t.accumulate(suns, sw_dir_cor_sum=acc_sw, sunlit_sum=acc_lit)
    tot_sw, tot_lit = R.fold(sh, sw, None, mask, fill)
    assert K.same(acc_sw, tot_sw) and K.same(acc_lit, tot_lit)
    f_cor, frac, _ = coarse(t, suns, (6, 20))
    own_f, own_l = K.block_means(sw, sh, mask, (6, 20), fill)
    assert K.same(f_cor, own_f) and K.same(frac, own_l)


DEGENERATE = (
    (((1, 1), (3, 3), (1, 1), 360, 5, "random", 105), (1,)),
    (((1, 130), (1, 130), (0, 0), 7, 5, "planar", 107), ((1, 13), (1, 130))),
)


@pytest.mark.parametrize("args,pixels", DEGENERATE)
def test_degenerate_grids(hip, args, pixels):
    c = R.make_case(*args)
    ref = R.reference(c)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    inside = ref["margin"] <= R.MARGIN
    for planes in (False, True):
        t = make(hip, c, planes)
        sh, sw = batch_maps(t, suns)
        for P in pixels:
            own_f, own_l = K.block_means(sw, sh, mask, P, fill)
            ref_f, ref_l = K.block_means(ref["val"], ref["code"], mask, P, fill)
            held = ~K.block_any(inside, P)
            assert (~held).sum() <= R.CAP * held.size, P
            for r in (0, 1):
                f_cor, frac, _ = coarse(t, suns, P, r=r)
                assert K.same(f_cor, own_f) and K.same(frac, own_l), (planes, P, r)
                assert K.same(f_cor[held], ref_f[held]) and K.same(frac[held], ref_l[held]), (planes, P, r)


def test_block_rows_wider_than_the_preferred_tile(hip):
    """Block rows of more than 512 cells: the fused kernel takes tiles of up to 4096 cells with fewer positions per pass."""
    c = R.make_case((2, 1040), (2, 1040), (0, 0), 7, 3, "planar", 305)
    c["mask"][0, 100:400] = 0
    ref = R.reference(c)
    mask, suns, fill = c["mask"], c["suns"], c["fill"]
    inside = ref["margin"] <= R.MARGIN
    for planes in (False, True):
        t = make(hip, c, planes)
        sh, sw = batch_maps(t, suns)
        for P in ((2, 520), (1, 1040), (2, 1040)):
            own_f, own_l = K.block_means(sw, sh, mask, P, fill)
            ref_f, ref_l = K.block_means(ref["val"], ref["code"], mask, P, fill)
            held = ~K.block_any(inside, P)
            assert (~held).sum() <= R.CAP * held.size, P
            f_cor, frac, _ = coarse(t, suns, P)
            f1, _, _ = coarse(t, suns, P, lit=False)
            _, l1, _ = coarse(t, suns, P, sw=False)
            assert K.same(f_cor, own_f) and K.same(frac, own_l) and K.same(f1, own_f) and K.same(l1, own_l), (planes, P)
            assert K.same(f_cor[held], ref_f[held]) and K.same(frac[held], ref_l[held]), (planes, P)
