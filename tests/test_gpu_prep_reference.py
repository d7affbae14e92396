"""The kernels of horayzon_amd/csrc/hz_prep.hip -- lonlat2ecef, ecef2enu, ecef2enu_vector, surf_norm, north_dir, wgs2swiss,
swiss2wgs, slope_plane_meth, slope_vector_meth, pack_vertices -- against tests/prep_reference.py (pinned to the golden
vectors by tests/test_prep_reference.py): at element counts around one workgroup, at the poles, the antimeridian,
longitudes outside (-180, 180], negative heights, Swiss-magnitude coordinates, the smallest grids, both slope branches,
and with dirty output buffers.  No bound is chosen in advance; each comes from the reference's own error on the case:

float64 outputs (ECEF X, Y, Z; LV95 e, n; lon, lat of swiss2wgs)
    |gpu - reference| <= 4 E.  E = max |float64 NumPy evaluation - reference| over the case, floored at one float64 ulp of
    the output's scale (6.4e6 m, 2.6e6 / 1.2e6 m, 1e2 degrees).  The factor 4: the device's sin / cos may be 2 ulp off
    where the host's are at most 1, and the chain of products doubles that again.
float32 outputs of float64 arithmetic (ecef2enu, ecef2enu_vector, surf_norm, north_dir, h_ch / h_wgs)
    |gpu - reference| <= ulp32(reference) / 2 + 4 E, componentwise: correctly rounded, except within the float64 slack of
    a rounding boundary.  Holds for components near zero, too.
slope kernels
    |gpu - float64 evaluation| <= 4 E32 + 2**-23, componentwise, E32 = max |float32 emulation - float64 evaluation| on the
    case (the floor covers the flat grid, where E32 = 0); the NaN pattern equals the reference's.  The number of words
    that differ from the float32 emulation is printed, not asserted.
pack_vertices
    np.array_equal with the reference.

Every figure is printed before it is asserted (pytest -s)."""
import os

import numpy as np
import pytest

from tests import prep_reference as R

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not R.HAVE_REFERENCE, reason=R.MISSING_PRECISION)

GOLD = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_reference.npz")))
HZ_OK, HZ_ERR_ARG = 0, 1
SURPLUS = 64
SENTINEL = -12345.6789
F64, F32 = np.float64, np.float32


def _f64(*arrays):
    return [R.to_float64(a) for a in arrays]


# ----------------------------------------------------------------------------------------------------------------------
# the one-lane-per-element kernels, each as: inputs(n), mirror(hip, inputs), abi(L, pointers ...), reference(inputs, T)
# ----------------------------------------------------------------------------------------------------------------------
class Kernel:
    """outs: [(name, dtype, floats per element, scale or None)] in the order mirror(), abi() and reference() use;
    arrays(inp): the input arrays abi() takes by pointer, in its order"""
    def __repr__(self):
        return self.name


class Lonlat2ecef(Kernel):
    outs = [("X", F64, 1, 6.4e6), ("Y", F64, 1, 6.4e6), ("Z", F64, 1, 6.4e6)]

    def __init__(self, ellps):
        self.ellps, self.kind, self.name = ellps, R.ELLPS[ellps], "lonlat2ecef-%s" % ellps

    def inputs(self, n):
        return R.geodetic_inputs(n)

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        return hip.transform.lonlat2ecef(*inp, ellps=self.ellps)

    def abi(self, L, i, n, o):
        return L.hz_lonlat2ecef(i[0], i[1], i[2], n, self.kind, o[0], o[1], o[2], 0)

    def reference(self, inp, T):
        return R.lonlat2ecef(*inp, self.kind, T)


class Ecef2enu(Kernel):
    outs = [("x_enu", F32, 1, None), ("y_enu", F32, 1, None), ("z_enu", F32, 1, None)]

    def __init__(self, ellps, lon_or, lat_or):
        self.ellps, self.kind, self.org = ellps, R.ELLPS[ellps], (lon_or, lat_or)
        self.name = "ecef2enu-%s-%g-%g" % (ellps, lon_or, lat_or)

    def inputs(self, n):
        lon, lat, h = R.patch_inputs(n, *self.org)
        return _f64(*R.lonlat2ecef(lon, lat, h, self.kind, F64))

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        T = hip.transform
        return T.ecef2enu(*inp, T.TransformerEcef2enu(lon_or=self.org[0], lat_or=self.org[1], ellps=self.ellps))

    def abi(self, L, i, n, o):
        return L.hz_ecef2enu(i[0], i[1], i[2], n, self.org[0], self.org[1], self.kind, o[0], o[1], o[2], 0)

    def reference(self, inp, T):
        return R.ecef2enu(*inp, self.kind, *self.org, T)


class Ecef2enuVector(Kernel):
    outs = [("vec_enu", F32, 3, None)]

    def __init__(self, ellps, lon_or, lat_or):
        self.ellps, self.kind, self.org = ellps, R.ELLPS[ellps], (lon_or, lat_or)
        self.name = "ecef2enu_vector-%s-%g-%g" % (ellps, lon_or, lat_or)

    def inputs(self, n):
        lon, lat, h = R.patch_inputs(n, *self.org)
        v = R.surf_norm(lon, lat, F64).astype(F32)
        if n >= 8:
            v[-4:] = ((1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, 0))
        return (v,)

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        T = hip.transform
        return (T.ecef2enu_vector(inp[0], T.TransformerEcef2enu(lon_or=self.org[0], lat_or=self.org[1], ellps=self.ellps)),)

    def abi(self, L, i, n, o):
        return L.hz_ecef2enu_vector(i[0], n, self.org[0], self.org[1], self.kind, o[0], 0)

    def reference(self, inp, T):
        return (R.ecef2enu_vector(inp[0], self.kind, *self.org, T),)


class SurfNorm(Kernel):
    name = "surf_norm"
    outs = [("vec_norm_ecef", F32, 3, None)]

    def inputs(self, n):
        return R.geodetic_inputs(n)[:2]

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        return (hip.direction.surf_norm(*inp),)

    def abi(self, L, i, n, o):
        return L.hz_surf_norm(i[0], i[1], n, o[0], 0)

    def reference(self, inp, T):
        return (R.surf_norm(*inp, T),)


class NorthDir(Kernel):
    outs = [("vec_north_ecef", F32, 3, None)]

    def __init__(self, ellps):
        self.ellps, self.kind, self.name = ellps, R.ELLPS[ellps], "north_dir-%s" % ellps

    def inputs(self, n):
        lon, lat, h = R.geodetic_inputs(n, lat_max=89.9)      # at the pole the projection is 0 / 0 in the reference too
        X, Y, Z = _f64(*R.lonlat2ecef(lon, lat, h, self.kind, F64))
        return X, Y, Z, R.surf_norm(lon, lat, F64).astype(F32)

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        return (hip.direction.north_dir(*inp, ellps=self.ellps),)

    def abi(self, L, i, n, o):
        return L.hz_north_dir(i[0], i[1], i[2], i[3], n, self.kind, o[0], 0)

    def reference(self, inp, T):
        return (R.north_dir(*inp, self.kind, T),)


class Wgs2swiss(Kernel):
    name = "wgs2swiss"
    outs = [("e", F64, 1, 2.6e6), ("n", F64, 1, 1.2e6), ("h_ch", F32, 1, None)]

    def inputs(self, n):
        return R.swiss_inputs(n)

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        return hip.transform.wgs2swiss(*inp)

    def abi(self, L, i, n, o):
        return L.hz_wgs2swiss(i[0], i[1], i[2], n, o[0], o[1], o[2], 0)

    def reference(self, inp, T):
        return R.wgs2swiss(*inp, T)


class Swiss2wgs(Kernel):
    """the round trip: its inputs are the (float64-evaluated) outputs of wgs2swiss on the same points"""
    name = "swiss2wgs"
    outs = [("lon", F64, 1, 1e2), ("lat", F64, 1, 1e2), ("h_wgs", F32, 1, None)]

    def inputs(self, n):
        e, no, h = R.wgs2swiss(*R.swiss_inputs(n), F64)
        return e, no, h.astype(F32)

    def arrays(self, inp):
        return list(inp)

    def mirror(self, hip, inp):
        return hip.transform.swiss2wgs(*inp)

    def abi(self, L, i, n, o):
        return L.hz_swiss2wgs(i[0], i[1], i[2], n, o[0], o[1], o[2], 0)

    def reference(self, inp, T):
        return R.swiss2wgs(*inp, T)


ORIGINS = (("WGS84", 8.0, 47.0), ("GRS80", -179.5, -60.0), ("sphere", 8.0, 47.0), ("WGS84", -179.5, -60.0))
KERNELS = ([Lonlat2ecef(e) for e in R.ELLPS_NAMES] + [Ecef2enu(*o) for o in ORIGINS] + [Ecef2enuVector(*o) for o in ORIGINS]
           + [SurfNorm()] + [NorthDir(e) for e in R.ELLPS_NAMES] + [Wgs2swiss(), Swiss2wgs()])


def _judge(kernel, n, got, inp):
    """the criteria of the module's docstring for every output of one call"""
    ref = kernel.reference(inp, R.REF_TYPE)
    yard = kernel.reference(inp, F64)
    for (name, dtype, width, scale), g, r, y in zip(kernel.outs, got, ref, yard):
        g = np.asarray(g)
        assert g.dtype == dtype and g.size == n * width, (kernel, name)
        g, r, y = g.reshape(-1), np.asarray(r).reshape(-1), np.asarray(y).reshape(-1)
        assert np.isfinite(g).all(), (kernel, name)
        if scale is None:
            scale = float(np.abs(R.to_float64(r)).max())
        E = max(float(R.abs_err(y, r).max()), float(np.spacing(max(scale, 2.0 ** -1000))))
        err = R.abs_err(g, r)
        if dtype == F64:
            worst, bound = float(err.max()), 4.0 * E
            print("%-34s n=%-6d %-14s E = %.3g  bound 4E = %.3g  gpu worst |error| = %.3g"
                  % (kernel, n, name, E, bound, worst))
            assert worst <= bound, (kernel, name)
        else:
            half = 0.5 * R.ulp32(r)
            excess = float((err - half).max())
            rounded = R.to_float64(r).astype(F32)
            print("%-34s n=%-6d %-14s E = %.3g  bound ulp32/2 + 4E, 4E = %.3g  gpu worst |error| - ulp32/2 = %.3g  "
                  "words that are not the rounded reference: %d of %d"
                  % (kernel, n, name, E, 4.0 * E, excess, int((g != rounded).sum()), g.size))
            assert (err <= half + 4.0 * E).all(), (kernel, name)


@needs_reference
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("kernel", KERNELS, ids=repr)
def test_elementwise_kernel_against_the_reference(hip, kernel, n):
    inp = kernel.inputs(n)
    _judge(kernel, n, kernel.mirror(hip, inp), inp)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32).ravel()


@pytest.mark.parametrize("kernel", KERNELS, ids=repr)
def test_device_pointers_give_the_host_words_and_leave_the_surplus(hip, kernel):
    """n = 257 (one lane past a workgroup) with every array in HBM and each output 64 elements longer than the kernel may
    write: the surplus keeps its sentinel, the rest is word for word what the call with host arrays returns."""
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    n = 257
    inp = kernel.inputs(n)
    host = kernel.mirror(hip, inp)
    dev_in = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in kernel.arrays(inp)]
    dev_out = [torch.full((n * width + SURPLUS,), SENTINEL, dtype=torch.float64 if dtype == F64 else torch.float32,
                          device="cuda:0") for _, dtype, width, _ in kernel.outs]
    torch.cuda.synchronize()
    rc = kernel.abi(_lib.lib(), [t.data_ptr() for t in dev_in], n, [t.data_ptr() for t in dev_out])
    _lib.check(rc)
    torch.cuda.synchronize()
    for (name, dtype, width, _), t, h in zip(kernel.outs, dev_out, host):
        got = t.cpu().numpy()
        assert np.array_equal(_words(got[n * width:]), _words(np.full(SURPLUS, SENTINEL, dtype))), (kernel, name)
        assert np.array_equal(_words(got[:n * width]), _words(h)), (kernel, name)


@pytest.mark.parametrize("kernel", KERNELS, ids=repr)
def test_no_elements_is_ok_and_writes_nothing(hip, kernel):
    from horayzon_amd import _lib
    inp = [np.ascontiguousarray(a) for a in kernel.arrays(kernel.inputs(4))]
    out = [np.full(4 * width, SENTINEL, dtype) for _, dtype, width, _ in kernel.outs]
    rc = kernel.abi(_lib.lib(), [a.ctypes.data for a in inp], 0, [a.ctypes.data for a in out])
    assert rc == HZ_OK
    for (name, dtype, width, _), a in zip(kernel.outs, out):
        assert np.array_equal(_words(a), _words(np.full(4 * width, SENTINEL, dtype))), (kernel, name)


# ----------------------------------------------------------------------------------------------------------------------
# slope
# ----------------------------------------------------------------------------------------------------------------------
SLOPE_CASES = list(R.slope_cases(GOLD))
SLOPE_REF = {"plane": R.slope_plane_meth, "vector": R.slope_vector_meth}


def _slope_gpu(hip, meth, x, y, z, rot, output_rot):
    fn = hip.topo_param.slope_plane_meth if meth == "plane" else hip.topo_param.slope_vector_meth
    return fn(x, y, z, rot_mat=rot, output_rot=output_rot)


def _ring(shape):
    ring = np.ones(shape, bool)
    ring[1:-1, 1:-1] = False
    return ring


@pytest.mark.parametrize("case", SLOPE_CASES, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_slope_kernel_against_the_reference(hip, case):
    name, meth, x, y, z, rot, output_rot = case
    got = _slope_gpu(hip, meth, x, y, z, rot, output_rot)
    f64 = SLOPE_REF[meth](x, y, z, rot, output_rot, T=F64)
    f32 = SLOPE_REF[meth](x, y, z, rot, output_rot, T=F32)
    assert got.dtype == F32 and got.shape == x.shape + (3,)
    ring = _ring(x.shape)
    assert np.isnan(got[ring]).all()                                   # the whole ring; everything below 3 x 3
    assert np.array_equal(np.isnan(got), np.isnan(f64))
    inner = ~ring
    if not inner.any():
        return
    e32 = float(np.abs(f32[inner].astype(F64) - f64[inner]).max())
    bound = 4.0 * e32 + 2.0 ** -23
    worst = float(np.abs(got[inner].astype(F64) - f64[inner]).max())
    differ = int((_words(got[inner]) != _words(f32[inner])).sum())
    print("slope_%-6s %-28s E32 = %.3g  bound 4 E32 + 2^-23 = %.3g  gpu worst |error| = %.3g  "
          "words that differ from the float32 emulation: %d of %d" % (meth, name, e32, bound, worst, differ, got[inner].size))
    assert (np.abs(got[inner].astype(F64) - f64[inner]) <= bound).all()
    if name == "flat":
        assert np.array_equal(got[inner], np.broadcast_to(np.array([0, 0, 1], F32), got[inner].shape))
    if name == "y_up_with_row":
        assert (got[inner][:, 2] > 0.0).all()                          # turned up by the flip branch


@pytest.mark.parametrize("meth", ("plane", "vector"))
@pytest.mark.parametrize("output_rot", (False, True))
def test_slope_interior_does_not_read_the_ring_of_rot_mat(hip, meth, output_rot):
    """rotation_matrix_glob2loc leaves the ring of rot_mat NaN; the interior must not depend on what stands there"""
    k = "WGS84_"
    x, y, z, rot = GOLD[k + "x_enu"], GOLD[k + "y_enu"], GOLD[k + "z_enu"], GOLD[k + "rot"]
    ring = _ring(x.shape)
    assert np.isnan(rot[ring]).all() and not np.isnan(rot[~ring]).any()
    filled = rot.copy()
    filled[ring] = np.eye(3, dtype=F32)
    a = _slope_gpu(hip, meth, x, y, z, rot, output_rot)
    b = _slope_gpu(hip, meth, x, y, z, filled, output_rot)
    assert not np.isnan(a[~ring]).any() and np.array_equal(_words(a[~ring]), _words(b[~ring]))


def test_slope_vector_zero_area_patch_is_nan(hip):
    x = np.full((3, 3), 5.0, F32)
    x[0, 0], x[0, 2], x[2, 0], x[2, 2] = 1.0, 2.0, 3.0, 4.0            # the corners are no stencil points
    got = hip.topo_param.slope_vector_meth(x, x.copy(), x.copy())
    assert np.isnan(got).all()


@pytest.mark.parametrize("meth", ("plane", "vector"))
def test_slope_device_pointers_give_the_host_words_and_leave_the_surplus(hip, meth):
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    L = _lib.lib()
    k = "GRS80_"
    x, y, z, rot = GOLD[k + "x_enu"], GOLD[k + "y_enu"], GOLD[k + "z_enu"], GOLD[k + "rot"]
    host = _slope_gpu(hip, meth, x, y, z, rot, True)
    dx, dy, dz, dr = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (x, y, z, rot))
    out = torch.full((x.size * 3 + SURPLUS,), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fn = L.hz_slope_plane_meth if meth == "plane" else L.hz_slope_vector_meth
    _lib.check(fn(dx.data_ptr(), dy.data_ptr(), dz.data_ptr(), x.shape[0], x.shape[1], dr.data_ptr(), 1, out.data_ptr(), 0))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_words(got[x.size * 3:]), _words(np.full(SURPLUS, SENTINEL, F32)))
    assert np.array_equal(_words(got[:x.size * 3]), _words(host))


# ----------------------------------------------------------------------------------------------------------------------
# pack_vertices
# ----------------------------------------------------------------------------------------------------------------------
PACK_SIZES = (1, 4, 5, 255, 256, 257, 65537)


def _planes(n):
    rng = np.random.default_rng(n)
    return [rng.uniform(-1e5, 1e5, n).astype(F32) for _ in range(3)]


@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_vertices_into_a_dirty_and_longer_buffer(hip, n):
    """the output starts as NaN and is four floats longer than hz_vert_grid_len(n): the kernel zeroes up to the length it
    is given, so the four are zero as well"""
    from horayzon_amd import _lib
    L = _lib.lib()
    assert L.hz_vert_grid_len(n) == R.vert_grid_len(n)
    x, y, z = _planes(n)
    out = np.full(R.vert_grid_len(n) + 4, np.nan, F32)
    _lib.check(L.hz_pack_vertices(x.ctypes.data, y.ctypes.data, z.ctypes.data, n, out.ctypes.data, out.size, 0))
    assert np.array_equal(out, R.pack_vertices(x, y, z, out.size))
    vg = hip.auxiliary.rearrange_pad_buffer(x.reshape(1, n), y.reshape(1, n), z.reshape(1, n))
    assert vg.dtype == F32 and np.array_equal(vg, R.pack_vertices(x, y, z))


def test_pack_vertices_device_tensors(hip):
    torch = pytest.importorskip("torch")
    from horayzon_amd import _lib
    n0, n1 = 7, 37                                                    # 259 vertices: past one workgroup
    x, y, z = (a.reshape(n0, n1) for a in _planes(n0 * n1))
    ref = R.pack_vertices(x, y, z)
    dev = [torch.from_numpy(a).to("cuda:0") for a in (x, y, z)]
    vg = hip.auxiliary.rearrange_pad_buffer(*dev)
    assert vg.device.type == "cuda" and vg.dtype == torch.float32 and np.array_equal(vg.cpu().numpy(), ref)
    # the same through the C ABI into a device buffer that held NaN, with a surplus the call is not told about
    out = torch.full((ref.size + SURPLUS,), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().hz_pack_vertices(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n0 * n1, out.data_ptr(),
                                          ref.size, 0))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:ref.size], ref) and np.isnan(got[ref.size:]).all()


@pytest.mark.parametrize("n", (1, 4, 257))
def test_pack_vertices_refuses_a_short_buffer(hip, n):
    from horayzon_amd import _lib
    x, y, z = _planes(n)
    out = np.full(R.vert_grid_len(n) - 1, np.nan, F32)
    rc = _lib.lib().hz_pack_vertices(x.ctypes.data, y.ctypes.data, z.ctypes.data, n, out.ctypes.data, out.size, 0)
    assert rc == HZ_ERR_ARG and np.isnan(out).all()
