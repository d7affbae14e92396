"""The 16-bit horizon code on the GPU (DESIGN.md section 4 clause 15; hz_q16.hip): quantise / dequantise,
horizon_gridded(hori_dtype="uint16"), and HorizonTerrain.initialise_q16.

Everything here is exact.  The code and the horizon call are compared word for word with the NumPy reference
(tests/q16_reference.py).  The look-up is held (a) to tests/horisun_reference.py evaluated on decode(encode(hori)) by the
rules of tests/test_gpu_horisun.py -- bit-identical outside the margin of 1e-9 rad, either decision inside, the cap asserted
(and asserted from the reference alone in tests/test_q16_reference.py) -- and (b) bit for bit to a float32 handle initialised
with decode(q): the kernel decodes to float32 before it widens, which is what makes (b) exact."""
import ctypes as C

import numpy as np
import pytest

from horayzon_amd.shadow import gridded_azimuths
from tests import horisun_reference as R
from tests import q16_reference as Q
from tests.test_gpu_horisun import batch_maps, same, weights_for
from tests.test_gpu_planes import ALL, horizon_case, knob, random_words

pytestmark = pytest.mark.gpu

LAYOUTS = ("cell_major", "azim_major")


def planes_of(a):
    return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def code_inputs():
    """(name, float32 array): the decoded code table, random 32-bit patterns, the small lengths and one of about 1e5."""
    table = Q.decode(np.arange(65536, dtype=np.uint32).astype(np.uint16))
    out = [("table", table), ("patterns", random_words((300, 331), seed=3))]
    for n in (1, 2, 3, 63, 64, 65, 257):
        out.append(("n%d" % n, random_words((n,), seed=n)))
    rng = np.random.default_rng(8)
    v = rng.uniform(-1.7, 1.7, 100003).astype(np.float32)
    v[::97] = np.nan
    v[1::97] = np.inf
    v[2::97] = -np.inf
    v[3::97] = -0.0
    out.append(("angles", v))
    return out


_CODE = {}


def code_cases():
    """Inputs and their reference codes, computed once and left unchanged."""
    if not _CODE:
        for name, v in code_inputs():
            _CODE[name] = (v, Q.encode(v))
    return _CODE


def as_u16(t):
    """A device tensor of codes (torch.uint16 or torch.int16) as a NumPy uint16 array."""
    import torch
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def same_f32(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the code --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", (-1, 100), ids=("one_chunk", "chunks_of_100"))
def test_quantise_and_dequantise_match_the_reference(hip, chunk):
    torch = pytest.importorskip("torch")
    H = hip.horizon
    with knob(b"q16_chunk", chunk, -1):
        for name, (v, want) in code_cases().items():
            q = H.quantise(v)
            assert isinstance(q, np.ndarray) and q.dtype == np.uint16 and q.shape == v.shape, name
            assert np.array_equal(q, want), name
            back = H.dequantise(q)
            assert same_f32(back, Q.decode(want)), name
            # device tensors in, device tensors out (moved as integers: no float compare touches a NaN)
            d_v = torch.from_numpy(v.view(np.int32)).to("cuda:0").view(torch.float32)
            torch.cuda.synchronize()
            d_q = H.quantise(d_v)
            assert isinstance(d_q, torch.Tensor) and d_q.is_cuda and tuple(d_q.shape) == v.shape, name
            assert str(d_q.dtype).split(".")[-1] in ("uint16", "int16")
            torch.cuda.synchronize()
            assert np.array_equal(as_u16(d_q), want), name
            d_back = H.dequantise(d_q)
            assert d_back.dtype == torch.float32
            torch.cuda.synchronize()
            assert np.array_equal(d_back.view(torch.int32).cpu().numpy().view(np.uint32), Q.decode(want).view(np.uint32)), name
            d_i16 = torch.from_numpy(want.view(np.int16)).to("cuda:0")          # int16 carrying the same bits
            torch.cuda.synchronize()
            d_back = H.dequantise(d_i16)
            torch.cuda.synchronize()
            assert np.array_equal(d_back.view(torch.int32).cpu().numpy().view(np.uint32), Q.decode(want).view(np.uint32)), name
    table = code_cases()["table"]
    assert np.array_equal(table[1], np.arange(65536, dtype=np.uint32).astype(np.uint16))     # encode(decode(q)) == q on the GPU
    assert (code_cases()["patterns"][1] == 0xFFFF).any()
    assert np.array_equal(H.quantise(np.zeros((0, 3), np.float32)), np.zeros((0, 3), np.uint16))


def test_mixed_sides_and_odd_offsets_through_the_c_abi(hip):
    """Host and device memory in all four combinations, in several staging chunks; and views at element 1 on either side:
    a destination of codes at 2 mod 4 bytes, a source of float32 at 4 mod 16."""
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    L = _lib.lib()
    v, want = code_cases()["angles"]
    n = v.size
    dec = Q.decode(want)
    d_v = torch.from_numpy(v.view(np.int32)).to("cuda:0")
    d_want = torch.from_numpy(want.view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    with knob(b"q16_chunk", 30001, -1):
        for src_dev in (False, True):
            for dst_dev in (False, True):
                q = np.zeros(n, np.uint16)
                d_q = torch.zeros(n, dtype=torch.int16, device="cuda:0")
                f = np.zeros(n, np.float32)
                d_f = torch.zeros(n, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                _lib.check(L.hz_hori_quantise(d_v.data_ptr() if src_dev else v.ctypes.data, n,
                                              d_q.data_ptr() if dst_dev else q.ctypes.data, 0))
                _lib.check(L.hz_hori_dequantise(d_want.data_ptr() if src_dev else want.ctypes.data, n,
                                                d_f.data_ptr() if dst_dev else f.ctypes.data, 0))
                torch.cuda.synchronize()
                got_q = as_u16(d_q) if dst_dev else q
                got_f = d_f.cpu().numpy().view(np.float32) if dst_dev else f
                assert np.array_equal(got_q, want), (src_dev, dst_dev)
                assert same_f32(got_f, dec), (src_dev, dst_dev)
    # views sliced at element 1 (and the words around them stay as they were)
    for m in (1, 2, 3, 4, 5, 9, 64, 1001):
        d_q = torch.full((m + 3,), 0x1234, dtype=torch.int16, device="cuda:0")
        d_f = torch.full((m + 3,), 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        view_q, view_f, view_v, view_w = d_q[1:m + 1], d_f[1:m + 1], d_v[1:m + 1], d_want[1:m + 1]
        assert view_q.data_ptr() % 4 == 2 and view_v.data_ptr() % 16 == 4
        _lib.check(L.hz_hori_quantise(view_v.data_ptr(), m, view_q.data_ptr(), 0))
        _lib.check(L.hz_hori_dequantise(view_w.data_ptr(), m, view_f.data_ptr(), 0))
        torch.cuda.synchronize()
        got_q, got_f = as_u16(d_q), d_f.cpu().numpy()
        assert np.array_equal(got_q[1:m + 1], want[1:m + 1]), m
        assert got_q[0] == 0x1234 and (got_q[m + 1:] == 0x1234).all(), m
        assert np.array_equal(got_f[1:m + 1].view(np.uint32), dec[1:m + 1].view(np.uint32)), m
        assert got_f[0] == 7 and (got_f[m + 1:] == 7).all(), m


# ---- 2. the horizon call ------------------------------------------------------------------------------------------

_FLOAT = {}


def narrow_case(cols):
    """horizon_case() with the inner domain cut to its first `cols` columns (63: rows of an odd number of cells)."""
    kw, tilt, par = horizon_case()
    if cols == kw["vec_norm"].shape[1]:
        return kw, tilt, par
    cut = lambda a: np.ascontiguousarray(a[:, :cols])             # noqa: E731
    kw = dict(kw, vec_norm=cut(kw["vec_norm"]), vec_north=cut(kw["vec_north"]))
    return kw, cut(tilt), dict(par, mask=cut(par["mask"]))


def float_result(hip, azim_num, layout, cols=64):
    """The float32 horizon call of the 60 x 72 case with all three maps, once per (azim_num, layout, columns)."""
    key = (azim_num, layout, cols)
    if key not in _FLOAT:
        kw, tilt, par = narrow_case(cols)
        hori, azim, maps = hip.horizon.horizon_gridded(**kw, **par, azim_num=azim_num, topo=ALL, topo_vec_tilt=tilt, layout=layout)
        _FLOAT[key] = (hori, azim, maps, dict(hip.horizon.last_stats))
    return _FLOAT[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("azim_num", (36, 5))
def test_horizon_call_writes_the_encoded_horizon(hip, azim_num, layout):
    kw, tilt, par = horizon_case()
    H = hip.horizon
    hori, azim, maps, st_f = float_result(hip, azim_num, layout)
    want = Q.encode(hori)
    assert (want == H.Q16_NAN).any()                              # masked cells: hori_fill = NaN
    chunk = 20                                                    # 52 rows: chunks of 20, 20 and 12
    q, azim_q, maps_q = H.horizon_gridded(**kw, **par, azim_num=azim_num, topo=ALL, topo_vec_tilt=tilt, layout=layout,
                                          hori_dtype="uint16", _chunk_rows=chunk)
    st = dict(H.last_stats)
    assert q.dtype == np.uint16 and q.shape == hori.shape and np.array_equal(q, want)
    assert np.array_equal(azim_q, azim)
    for name in ALL:
        assert same_f32(maps_q[name], maps[name]), name           # reduced from the unquantised chunk
    assert st["num_rays"] == st_f["num_rays"] and st["num_cells"] == st_f["num_cells"]
    cells = chunk * kw["vec_norm"].shape[1]
    assert st["scratch_bytes"] >= cells * azim_num * (4 + 2)      # the float32 chunk buffer and the one of codes
    # without topo, in one chunk
    plain, _ = H.horizon_gridded(**kw, **par, azim_num=azim_num, layout=layout, hori_dtype="uint16")
    assert np.array_equal(plain, want)


def test_horizon_call_rows_scene_and_devices(hip):
    kw, tilt, par = horizon_case()
    H = hip.horizon
    A = 36
    b, e = 9, 41                                                  # strictly inside; 32 rows in chunks of 12, 12 and 8
    sc = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])
    for layout in LAYOUTS:
        want = Q.encode(float_result(hip, A, layout)[0])
        rows = (lambda a: a[:, b:e]) if layout == "azim_major" else (lambda a: a[b:e])
        part, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout=layout, hori_dtype="uint16", rows=(b, e), _chunk_rows=12)
        assert part.dtype == np.uint16 and np.array_equal(rows(part), rows(want))
        outside = part.copy()
        rows(outside)[...] = H.Q16_NAN
        assert (outside == H.Q16_NAN).all() and not (rows(part) == H.Q16_NAN).all()
        on_scene, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout=layout, hori_dtype="uint16", scene=sc, _chunk_rows=20)
        assert np.array_equal(on_scene, want)
        two, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout=layout, hori_dtype="uint16", devices=[0, 0], _chunk_rows=7)
        assert np.array_equal(two, want)
    sc.close()


@pytest.mark.parametrize("cols", (64, 63))
def test_horizon_call_device_resident_codes(hip, cols):
    """hz_horizon_gridded_scene_q16 with hori_q in HBM, both layouts: the whole domain, a slab with hori_is_slab (a plane
    stride of 26 rows x 64 columns, and of 25 rows x 63 columns: odd), each also through a view at element 1 (the codes start
    at 2 mod 4 bytes), and a slab inside whole-domain codes (63 columns: it starts at an odd cell)."""
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    kw, tilt, par = narrow_case(cols)
    A = 24
    hori, azim, maps, _ = float_result(hip, A, "cell_major", cols)
    in0, in1 = hori.shape[:2]
    sc = hip.Scene.create(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_norm = torch.from_numpy(kw["vec_norm"]).to(dev)
    d_north = torch.from_numpy(kw["vec_north"]).to(dev)
    d_mask = torch.from_numpy(par["mask"]).to(dev)
    d_tilt = torch.from_numpy(tilt).to(dev)
    SENTINEL = 0x1234

    def call(planes, rb, re, slab, chunk, shift=0):
        n_out = re - rb if slab else in0
        shape = (A, n_out, in1) if planes else (n_out, in1, A)
        flat = torch.full((A * n_out * in1 + shift,), SENTINEL, dtype=torch.int16, device=dev)
        d_q = flat[shift:]                                        # shift = 1: the codes start at 2 mod 4 bytes
        d_svf, d_vsf, d_open = (torch.full((n_out, in1), 7.0, dtype=torch.float32, device=dev) for _ in range(3))
        torch.cuda.synchronize()
        o = _lib.hz_opts()
        o.device = sc.device
        o.row_begin, o.row_end = rb, re
        o.hori_is_slab = int(slab)
        o.chunk_rows = chunk
        o.vec_tilt = d_tilt.data_ptr()
        o.svf = d_svf.data_ptr()
        t = _lib.hz_topo_out(d_vsf.data_ptr(), d_open.data_ptr())
        st = _lib.hz_stats()
        _lib.check(L.hz_horizon_gridded_scene_q16(sc._h, d_norm.data_ptr(), d_north.data_ptr(), kw["offset_0"], kw["offset_1"],
                                                  d_q.data_ptr(), int(planes), in0, in1, A, par["dist_search"], 0.25,
                                                  b"guess_constant", par["elev_ang_low_lim"], d_mask.data_ptr(),
                                                  par["hori_fill"], 0.01, C.byref(o), C.byref(t), C.byref(st)))
        torch.cuda.synchronize()
        assert shift == 0 or flat[0].item() == SENTINEL
        return {"q": as_u16(d_q).reshape(shape), "svf": d_svf.cpu().numpy(), "vsf": d_vsf.cpu().numpy(),
                "openness": d_open.cpu().numpy()}

    rb, re = (11, 37) if cols == 64 else (11, 36)
    for planes in (0, 1):
        want = Q.encode(planes_of(hori) if planes else hori)
        rows = (lambda a: a[:, rb:re]) if planes else (lambda a: a[rb:re])
        whole = call(planes, 0, in0, False, 20)
        assert np.array_equal(whole["q"], want)
        for name in ALL:
            assert same_f32(whole[name], maps[name]), name
        for shift in (0, 1):
            slab = call(planes, rb, re, True, 10, shift)          # the codes hold the slab's rows only
            assert np.array_equal(slab["q"], rows(want)), (planes, shift)
            for name in ALL:
                assert same_f32(slab[name], np.ascontiguousarray(maps[name][rb:re])), name
        inside = call(planes, rb, re, False, 10)                  # whole-domain codes, rows outside the slab untouched
        assert np.array_equal(rows(inside["q"]), rows(want))
        rest = inside["q"].copy()
        rows(rest)[...] = SENTINEL
        assert (rest == SENTINEL).all()
    sc.close()


def test_horizon_call_rows_of_an_odd_number_of_cells(hip):
    """52 x 63 cells: chunks of 5 rows are 315 cells, an odd plane stride in the chunk buffer of codes, and the slab starts
    at the odd cell 11 * 63 of every plane -- the 4-byte boundaries alternate from plane to plane."""
    kw, tilt, par = narrow_case(63)
    H = hip.horizon
    A = 33                                                        # one azimuth beyond the tile's 32
    b, e = 11, 36
    for layout in LAYOUTS:
        want = Q.encode(float_result(hip, A, layout, 63)[0])
        rows = (lambda a: a[:, b:e]) if layout == "azim_major" else (lambda a: a[b:e])
        q, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout=layout, hori_dtype="uint16", _chunk_rows=5)
        assert np.array_equal(q, want), layout
        part, _ = H.horizon_gridded(**kw, **par, azim_num=A, layout=layout, hori_dtype="uint16", rows=(b, e), _chunk_rows=5)
        assert np.array_equal(rows(part), rows(want)), layout
        rows(part)[...] = H.Q16_NAN
        assert (part == H.Q16_NAN).all()


# ---- 3. the look-up against the reference -------------------------------------------------------------------------

_REF = {}


def ref_of(name):
    """(case with hori = decode(q), q, reference on that horizon), computed once per session and left unchanged."""
    if name not in _REF:
        c = Q.case(name)
        q = Q.encode(c["hori"])
        c["hori"] = Q.decode(q)
        _REF[name] = (c, q, R.reference(c))
    return _REF[name]


def terrain_q16(hip, c, q, layout, device_tensor=False):
    hori_q = planes_of(q) if layout == "azim_major" else q
    if device_tensor:
        import torch
        hori_q = torch.from_numpy(hori_q.view(np.int16)).to("cuda:0")
        torch.cuda.synchronize()
    t = hip.shadow.HorizonTerrain()
    t.initialise_q16(gridded_azimuths(c["azim_num"]), hori_q, c["vert_grid"], c["dem_dim_0"], c["dem_dim_1"], c["offset_0"],
                     c["offset_1"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], c["mask"],
                     sw_dir_cor_fill=c["fill"], ang_max=c["ang_max"], layout=layout)
    return t


def terrain_f32(hip, c, layout):
    t = hip.shadow.HorizonTerrain()
    init = t.initialise_azim_major if layout == "azim_major" else t.initialise
    init(gridded_azimuths(c["azim_num"]), planes_of(c["hori"]) if layout == "azim_major" else c["hori"], c["vert_grid"],
         c["dem_dim_0"], c["dem_dim_1"], c["offset_0"], c["offset_1"], c["vec_tilt"], c["vec_norm"], c["vec_north"],
         c["surf_enl_fac"], c["mask"], sw_dir_cor_fill=c["fill"], ang_max=c["ang_max"])
    return t


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_look_up_matches_the_reference(hip, name, layout):
    c, q, ref = ref_of(name)
    mask, suns = c["mask"], c["suns"]
    S = suns.shape[0]
    t = terrain_q16(hip, c, q, layout)
    with knob(b"horisun_chunk", R.CHUNK_TEST, -1):             # S = 5 runs in two launches
        sh, sw = batch_maps(t, suns, mask.shape)
        w = weights_for(S)
        sum_sw = np.full(mask.shape, 77.0, np.float32)
        sum_lit = np.full(mask.shape, 77.0, np.float32)
        t.accumulate(suns, w, sw_dir_cor_sum=sum_sw, sunlit_sum=sum_lit)
    inside = ref["margin"] <= R.MARGIN
    unmasked_pairs = int((mask == 1).sum()) * S
    flips = int(((sh != ref["code"]) & inside).sum())
    print("%s %s: %d unmasked pairs, %d inside the margin, %d of them decided the other way, smallest margin %.3g rad"
          % (name, layout, unmasked_pairs, int(inside.sum()), flips, float(ref["margin"].min())))
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
    # accumulate: the clause 9 fold of the GPU's own maps, bit for bit; and the reference's fold where no pair of the cell is inside
    own_sw, own_lit = R.fold(sh, sw, w, mask, c["fill"])
    assert same(sum_sw, own_sw) and same(sum_lit, own_lit)
    ref_sw, ref_lit = R.fold(ref["code"], ref["val"], w, mask, c["fill"])
    clean = ~inside.any(axis=0)
    assert same(sum_sw[clean], ref_sw[clean]) and same(sum_lit[clean], ref_lit[clean])
    assert np.isnan(sum_sw[mask != 1]).all() and np.isnan(sum_lit[mask != 1]).all()


# ---- 4. the look-up against the float handle ----------------------------------------------------------------------

def divisor_pair(shape):
    """A block that divides the inner domain and is not 1 x 1 where the domain allows one."""
    small = lambda n: next((d for d in (2, 3, 5, 7, 13, 37, 53) if n % d == 0 and d <= n), 1)      # noqa: E731
    return small(shape[0]), small(shape[1])


def every_output(t, c):
    """Every method's output as bytes: the batch maps and sums, sun_times over a track of 5 positions, and
    sw_dir_cor_coarse for blocks 1 x 1 and a divisor pair under both values of the route knob."""
    mask = c["mask"]
    shape = mask.shape
    out = {}
    track = c["suns"] if c["suns"].shape[0] == 5 else np.ascontiguousarray(np.repeat(c["suns"], 5, axis=0)
                                                                           + np.arange(5, dtype=np.float32)[:, None] * np.float32(3.0e9))
    times = np.arange(5, dtype=np.float64) * 600.0 + 7.0
    S = c["suns"].shape[0]
    with knob(b"horisun_chunk", R.CHUNK_TEST, -1):
        out["sh"], out["sw"] = batch_maps(t, c["suns"], shape)
        out["sum_sw"], out["sum_lit"] = np.full(shape, 77.0, np.float32), np.full(shape, 77.0, np.float32)
        t.accumulate(c["suns"], weights_for(S), sw_dir_cor_sum=out["sum_sw"], sunlit_sum=out["sum_lit"])
        st = dict(sunrise=np.full(shape, 77.0, np.float32), sunset=np.full(shape, 77.0, np.float32),
                  duration=np.full(shape, 77.0, np.float32), intervals=np.full(shape, 77, np.int32))
        t.sun_times(track, times, **st)
        out.update(st)
        for blocks in ((1, 1), divisor_pair(shape)):
            for route in (0, 1):
                with knob(b"horisun_coarse_route", route, -1):
                    g = (S, shape[0] // blocks[0], shape[1] // blocks[1])
                    f_cor, frac = np.full(g, 77.0, np.float32), np.full(g, 77.0, np.float32)
                    t.sw_dir_cor_coarse(c["suns"], blocks, f_cor=f_cor, sunlit_frac=frac)
                    out["f_cor_%dx%d_r%d" % (blocks + (route,))] = f_cor
                    out["frac_%dx%d_r%d" % (blocks + (route,))] = frac
    return {k: v.tobytes() for k, v in out.items()}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ("inner_A360_planar", "inner_A7_random", "cell_A1_planar", "row_A2_planar"))
def test_look_up_equals_the_float_handle_on_the_decoded_horizon(hip, name, layout):
    c, q, _ = ref_of(name)
    assert np.isnan(c["hori"]).any() or c["hori"].size < 50      # the reserved code takes part
    elevation = np.ascontiguousarray(c["vert"][..., 2])
    tf, tq = terrain_f32(hip, c, layout), terrain_q16(hip, c, q, layout)
    want, got = every_output(tf, c), every_output(tq, c)
    assert sorted(want) == sorted(got)
    for key in want:
        assert want[key] == got[key], key
    # the route knob is ignored for codes: both routes gave the float handle's words, and its two routes agree
    for key in want:
        if key.endswith("_r0"):
            assert want[key] == want[key[:-1] + "1"], key
    tf.refraction(elevation)
    tq.refraction(elevation)
    assert tq.refrac_cor
    want_r, got_r = every_output(tf, c), every_output(tq, c)
    for key in want_r:
        assert want_r[key] == got_r[key], "refracted " + key
    if name.startswith("inner"):
        assert want_r["sh"] != want["sh"] or want_r["sw"] != want["sw"]        # the refraction did move something
    # initialise_q16 switches the refraction off again
    tq2 = terrain_q16(hip, c, q, layout)
    assert not tq2.refrac_cor


@pytest.mark.parametrize("layout", LAYOUTS)
def test_borrowed_device_codes_give_the_same_bytes(hip, layout):
    pytest.importorskip("torch")
    c, q, _ = ref_of("inner_A7_random")
    host = every_output(terrain_q16(hip, c, q, layout), c)
    td = terrain_q16(hip, c, q, layout, device_tensor=True)
    assert td._hori is not None and td._hori.is_cuda             # borrowed: the object holds a reference
    dev = every_output(td, c)
    for key in host:
        assert host[key] == dev[key], key
