"""NumPy restatement of the input-preparation and slope kernels (horayzon_amd/csrc/hz_prep.hip, with the host set-up of
make_ellps / make_frame and the length rule of hz_vert_grid_len in include/horayzon_hip.h), statement by statement, in two
precisions each.  It imports neither the library nor a GPU and reads no file: tests/test_prep_reference.py pins it to the
golden vectors, tests/test_gpu_prep_reference.py holds the kernels to it.

float64 kernels (lonlat2ecef, ecef2enu, ecef2enu_vector, surf_norm, north_dir, wgs2swiss, swiss2wgs)
    one function each with a type parameter T: np.float64 is the yardstick (the kernel's own arithmetic on the host),
    REF_TYPE the reference: np.longdouble where it has 64 mantissa bits (LONGDOUBLE_OK), else the 113-bit mpmath context MP,
    else None (HAVE_REFERENCE False; tests that need the reference skip with MISSING_PRECISION as the reason).  Every
    literal of the kernel enters as the double the compiler makes of it and is widened, degree -> radian included.

float32 kernels (slope_plane_meth, slope_vector_meth)
    T = np.float64 is the evaluation, T = np.float32 the emulation: NumPy rounds each elementwise operation to the array's
    type and never contracts a product into a sum, so the same statements in the kernel's order give the kernel's words
    (the library is built with -ffp-contract=off; float32 division and square root are correctly rounded on both sides).
    Vectorised over the interior cells.

pack_vertices
    interleave and pad; vert_grid_len restates the rule of the header: 16 extra floats, plus what makes the byte size a
    multiple of 16."""
import numpy as np

try:
    import mpmath
except Exception:                                     # pragma: no cover - depends on the machine
    mpmath = None

LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
ELLPS = {"sphere": 0, "GRS80": 1, "WGS84": 2}
ELLPS_NAMES = tuple(ELLPS)


class _Mp:
    """113-bit mpmath arithmetic on object arrays: what REF_TYPE is where np.longdouble is only a double."""

    def __init__(self):
        self.ctx = mpmath.mp.clone()
        self.ctx.prec = 113
        self._mpf = np.frompyfunc(self.ctx.mpf, 1, 1)
        self.sin = np.frompyfunc(self.ctx.sin, 1, 1)
        self.cos = np.frompyfunc(self.ctx.cos, 1, 1)
        self.sqrt = np.frompyfunc(self.ctx.sqrt, 1, 1)

    def arr(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        hi = a.astype(np.float64)
        if a.dtype != np.longdouble:
            return self._mpf(hi)
        return self._mpf(hi) + self._mpf((a - hi).astype(np.float64))     # a long double is the sum of two doubles

    def __repr__(self):
        return "mpmath(prec=113)"


class _Np:
    sin, cos, sqrt = np.sin, np.cos, np.sqrt

    def __init__(self, T):
        self.T = T

    def arr(self, a):
        return np.asarray(a).astype(self.T)


MP = _Mp() if mpmath is not None else None
REF_TYPE = np.longdouble if LONGDOUBLE_OK else MP
HAVE_REFERENCE = REF_TYPE is not None
MISSING_PRECISION = ("no reference precision beyond float64: np.longdouble has eps %.3g > 2**-63 on this machine and "
                     "mpmath does not import" % float(np.finfo(np.longdouble).eps))


def _prec(T):
    return T if isinstance(T, _Mp) else _Np(T)


def to_float64(a):
    """an array of any of the types above, rounded to float64"""
    a = np.asarray(a)
    return np.array([float(v) for v in a.ravel()], np.float64).reshape(a.shape) if a.dtype == object else a.astype(np.float64)


def abs_err(got, ref):
    """|got - ref| evaluated in the type of `ref` (the wider one), returned as float64"""
    ref = np.asarray(ref)
    got = np.asarray(got)
    if ref.dtype == object:
        return to_float64(np.abs(MP.arr(got) - ref))
    return np.abs(got.astype(ref.dtype) - ref).astype(np.float64)


def ulp32(ref):
    """one float32 unit in the last place at |ref|, from the binade of the value itself (not of its rounded float32, which
    near a power of two would double it); 2**-149 below the normal range and at zero"""
    m, e = np.frexp(np.abs(to_float64(ref)))                      # |x| = m * 2**e, m in [0.5, 1)
    return np.where(m == 0.0, 2.0 ** -149, np.maximum(np.ldexp(1.0, e - 24), 2.0 ** -149))


# ------------------------------------------------------------------------------------------------------------------
# float64 kernels
# ------------------------------------------------------------------------------------------------------------------
def _deg2rad(P):
    return P.arr(np.float64(3.14159265358979323846) / np.float64(180.0))      # deg2rad_d: one double constant, widened


def make_ellps(kind, T):
    """make_ellps: (sphere, r, a, b, e_2)"""
    P = _prec(T)
    c = lambda v: P.arr(np.float64(v))
    r, a = c(6370997.0), c(6378137.0)
    f = (c(1.0) / c(298.257222101)) if kind == 1 else (c(1.0) / c(298.257223563))
    b = a * (c(1.0) - f)
    e_2 = c(1.0) - ((b * b) / (a * a))
    return kind == 0, r, a, b, e_2


def lonlat2ecef(lon, lat, h, kind, T):
    """lonlat2ecef_one: lon, lat float64 [degree], h float32 -> X, Y, Z"""
    P = _prec(T)
    sphere, r, a, b, e_2 = make_ellps(kind, T)
    d = _deg2rad(P)
    lon, lat, h = P.arr(lon), P.arr(lat), P.arr(h)
    sl, cl = P.sin(lat * d), P.cos(lat * d)
    so, co = P.sin(lon * d), P.cos(lon * d)
    if sphere:
        return (r + h) * cl * co, (r + h) * cl * so, (r + h) * sl
    n = a / P.sqrt(P.arr(np.float64(1.0)) - e_2 * (sl * sl))
    return (n + h) * cl * co, (n + h) * cl * so, ((b * b) / (a * a) * n + h) * sl


def make_frame(kind, lon_or, lat_or, T):
    """make_frame: (sin_lon, cos_lon, sin_lat, cos_lat, x_or, y_or, z_or)"""
    P = _prec(T)
    sphere, r, a, b, e_2 = make_ellps(kind, T)
    d = P.arr(np.float64(np.pi) / np.float64(180.0))                           # M_PI / 180.0
    lo, la = P.arr(np.float64(lon_or)) * d, P.arr(np.float64(lat_or)) * d
    sin, cos = P.sin, P.cos
    if sphere:
        x_or, y_or, z_or = r * cos(la) * cos(lo), r * cos(la) * sin(lo), r * sin(la)
    else:
        n = a / P.sqrt(P.arr(np.float64(1.0)) - e_2 * (sin(la) * sin(la)))
        x_or, y_or = n * cos(la) * cos(lo), n * cos(la) * sin(lo)
        z_or = ((b * b) / (a * a) * n) * sin(la)
    return sin(lo), cos(lo), sin(la), cos(la), x_or, y_or, z_or


def ecef2enu(X, Y, Z, kind, lon_or, lat_or, T):
    """k_ecef2enu before its rounding to float32"""
    P = _prec(T)
    sin_lon, cos_lon, sin_lat, cos_lat, x_or, y_or, z_or = make_frame(kind, lon_or, lat_or, T)
    dx, dy, dz = P.arr(X) - x_or, P.arr(Y) - y_or, P.arr(Z) - z_or
    return (-sin_lon * dx + cos_lon * dy,
            -sin_lat * cos_lon * dx - sin_lat * sin_lon * dy + cos_lat * dz,
            +cos_lat * cos_lon * dx + cos_lat * sin_lon * dy + sin_lat * dz)


def ecef2enu_vector(v, kind, lon_or, lat_or, T):
    """k_ecef2enu_vector before its rounding to float32: v float32 (n, 3) -> (n, 3)"""
    P = _prec(T)
    sin_lon, cos_lon, sin_lat, cos_lat = make_frame(kind, lon_or, lat_or, T)[:4]
    v = P.arr(v)
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([-sin_lon * a + cos_lon * b,
                     -sin_lat * cos_lon * a - sin_lat * sin_lon * b + cos_lat * c,
                     +cos_lat * cos_lon * a + cos_lat * sin_lon * b + sin_lat * c], axis=1)


def surf_norm(lon, lat, T):
    """k_surf_norm before its rounding to float32: -> (n, 3)"""
    P = _prec(T)
    d = _deg2rad(P)
    lon, lat = P.arr(lon), P.arr(lat)
    so, co = P.sin(lon * d), P.cos(lon * d)
    sl, cl = P.sin(lat * d), P.cos(lat * d)
    return np.stack([cl * co, cl * so, sl], axis=1)


def north_dir(X, Y, Z, vn, kind, T):
    """k_north_dir before its rounding to float32 (np_z = r on the sphere, else b): vn float32 (n, 3) -> (n, 3)"""
    P = _prec(T)
    sphere, r, a, b, e_2 = make_ellps(kind, T)
    np_z = r if sphere else b
    zero = P.arr(np.float64(0.0))
    vx, vy, vz = zero - P.arr(X), zero - P.arr(Y), np_z - P.arr(Z)
    vn = P.arr(vn)
    nx, ny, nz = vn[:, 0], vn[:, 1], vn[:, 2]
    dot = (vx * nx) + (vy * ny) + (vz * nz)
    px, py, pz = vx - dot * nx, vy - dot * ny, vz - dot * nz
    norm = P.sqrt(px * px + py * py + pz * pz)
    return np.stack([px / norm, py / norm, pz / norm], axis=1)


def wgs2swiss(lon, lat, h_wgs, T):
    """k_wgs2swiss: -> e, n (float64 outputs) and h_ch before its rounding to float32"""
    P = _prec(T)
    c = lambda v: P.arr(np.float64(v))
    lon, lat, h_wgs = P.arr(lon), P.arr(lat), P.arr(h_wgs)
    lo = ((lon * c(3600.0)) - c(26782.5)) / c(10000.0)
    la = ((lat * c(3600.0)) - c(169028.66)) / c(10000.0)
    e = c(2600072.37) + c(211455.93) * lo - c(10938.51) * lo * la - c(0.36) * lo * (la * la) - c(44.54) * (lo * lo * lo)
    n = (c(1200147.07) + c(308807.95) * la + c(3745.25) * (lo * lo) + c(76.63) * (la * la) - c(194.56) * (lo * lo) * la
         + c(119.79) * (la * la * la))
    h_ch = h_wgs - c(49.55) + c(2.73) * lo + c(6.94) * la
    return e, n, h_ch


def swiss2wgs(e, n, h_ch, T):
    """k_swiss2wgs: -> lon, lat (float64 outputs) and h_wgs before its rounding to float32"""
    P = _prec(T)
    c = lambda v: P.arr(np.float64(v))
    e, n, h_ch = P.arr(e), P.arr(n), P.arr(h_ch)
    ep, np_ = (e - c(2600000.0)) / c(1000000.0), (n - c(1200000.0)) / c(1000000.0)
    lo = c(2.6779094) + c(4.728982) * ep + c(0.791484) * ep * np_ + c(0.1306) * ep * (np_ * np_) - c(0.0436) * (ep * ep * ep)
    la = (c(16.9023892) + c(3.238272) * np_ - c(0.270978) * (ep * ep) - c(0.002528) * (np_ * np_) - c(0.0447) * (ep * ep) * np_
          - c(0.0140) * (np_ * np_ * np_))
    h_wgs = h_ch + c(49.55) - c(12.60) * ep - c(22.64) * np_
    return lo * (c(100.0) / c(36.0)), la * (c(100.0) / c(36.0)), h_wgs


# ------------------------------------------------------------------------------------------------------------------
# float32 kernels: slope
# ------------------------------------------------------------------------------------------------------------------
def _ring_nan(shape, T):
    return np.full(tuple(shape) + (3,), np.nan, T)


def slope_plane_meth(x, y, z, rot_mat=None, output_rot=False, T=np.float64):
    """k_slope_plane: x, y, z float32 (len_0, len_1), rot_mat float32 (len_0, len_1, 3, 3) or None -> (len_0, len_1, 3) of
    type T, NaN on the outermost ring.  T = np.float32 gives the kernel's words."""
    len_0, len_1 = x.shape
    out = _ring_nan(x.shape, T)
    if len_0 < 3 or len_1 < 3:
        return out
    x, y, z = (np.asarray(v).astype(T) for v in (x, y, z))
    inner = (slice(1, -1), slice(1, -1))
    m = (len_0 - 2) * (len_1 - 2)
    if rot_mat is None:
        r = [np.full(m, v, T) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1)]
    else:
        rm = np.asarray(rot_mat).astype(T)[inner].reshape(m, 9)
        r = [rm[:, k] for k in range(9)]
    xc, yc, zc = x[inner].ravel(), y[inner].ravel(), z[inner].ravel()
    zero = np.zeros(m, T)
    x_l_sum, y_l_sum, z_l_sum, xx, xy, xz, yy, yz = (zero.copy() for _ in range(8))
    for k in range(3):                                             # k = i - 1 .. i + 1
        for l in range(3):                                         # l = j - 1 .. j + 1: row-major
            q = (slice(k, len_0 - 2 + k), slice(l, len_1 - 2 + l))
            cx, cy, cz = x[q].ravel() - xc, y[q].ravel() - yc, z[q].ravel() - zc
            vx = r[0] * cx + r[1] * cy + r[2] * cz
            vy = r[3] * cx + r[4] * cy + r[5] * cz
            vz = r[6] * cx + r[7] * cy + r[8] * cz
            x_l_sum = x_l_sum + vx; y_l_sum = y_l_sum + vy; z_l_sum = z_l_sum + vz
            xx = xx + vx * vx; xy = xy + vx * vy; xz = xz + vx * vz; yy = yy + vy * vy; yz = yz + vy * vz
    A = [[xx, xy, x_l_sum], [xy, yy, y_l_sum], [x_l_sum, y_l_sum, np.full(m, 9, T)]]
    b = [xz, yz, z_l_sum]
    with np.errstate(all="ignore"):
        for col in range(3):                                       # LU with partial pivoting, the kernel's `>`
            piv = np.full(m, col)
            best = np.abs(A[col][col])
            for row in range(col + 1, 3):
                gt = np.abs(A[row][col]) > best
                best = np.where(gt, np.abs(A[row][col]), best)
                piv = np.where(gt, row, piv)
            for row in range(col + 1, 3):                          # swap rows col <-> piv where piv == row
                sw = piv == row
                for k in range(3):
                    A[col][k], A[row][k] = np.where(sw, A[row][k], A[col][k]), np.where(sw, A[col][k], A[row][k])
                b[col], b[row] = np.where(sw, b[row], b[col]), np.where(sw, b[col], b[row])
            inv = np.ones(m, T) / A[col][col]
            for row in range(col + 1, 3):
                f = A[row][col] * inv
                for k in range(col + 1, 3):
                    A[row][k] = A[row][k] - f * A[col][k]
                b[row] = b[row] - f * b[col]
        s1 = (b[1] - A[1][2] * (b[2] / A[2][2])) / A[1][1]
        s0 = (b[0] - A[0][1] * s1 - A[0][2] * (b[2] / A[2][2])) / A[0][0]
        vx, vy, vz = s0, s1, np.full(m, -1, T)
        mag = np.sqrt(vx * vx + vy * vy + vz * vz)
        vx, vy, vz = vx / mag, vy / mag, vz / mag
        flip = vz < 0
        vx, vy, vz = np.where(flip, -vx, vx), np.where(flip, -vy, vy), np.where(flip, -vz, vz)
        if not output_rot:                                         # back with the transpose
            vx, vy, vz = (r[0] * vx + r[3] * vy + r[6] * vz,
                          r[1] * vx + r[4] * vy + r[7] * vz,
                          r[2] * vx + r[5] * vy + r[8] * vz)
    out[inner] = np.stack([vx, vy, vz], axis=1).reshape(len_0 - 2, len_1 - 2, 3)
    return out


def slope_vector_meth(x, y, z, rot_mat=None, output_rot=False, T=np.float64):
    """k_slope_vector: arguments and result as slope_plane_meth"""
    len_0, len_1 = x.shape
    out = _ring_nan(x.shape, T)
    if len_0 < 3 or len_1 < 3:
        return out
    x, y, z = (np.asarray(v).astype(T) for v in (x, y, z))
    c = (slice(1, -1), slice(1, -1))
    w, e = (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))
    s, n = (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1))
    a_x, a_y, a_z = x[w] - x[c], y[w] - y[c], z[w] - z[c]
    b_x, b_y, b_z = x[s] - x[c], y[s] - y[c], z[s] - z[c]
    c_x, c_y, c_z = x[e] - x[c], y[e] - y[c], z[e] - z[c]
    d_x, d_y, d_z = x[n] - x[c], y[n] - y[c], z[n] - z[c]
    four = T(4.0)
    with np.errstate(all="ignore"):
        vx = ((a_y * b_z - a_z * b_y) + (b_y * c_z - b_z * c_y) + (c_y * d_z - c_z * d_y) + (d_y * a_z - d_z * a_y)) / four
        vy = ((a_z * b_x - a_x * b_z) + (b_z * c_x - b_x * c_z) + (c_z * d_x - c_x * d_z) + (d_z * a_x - d_x * a_z)) / four
        vz = ((a_x * b_y - a_y * b_x) + (b_x * c_y - b_y * c_x) + (c_x * d_y - c_y * d_x) + (d_x * a_y - d_y * a_x)) / four
        mag = np.sqrt(vx * vx + vy * vy + vz * vz)
        vx, vy, vz = vx / mag, vy / mag, vz / mag
        flip = vz < 0
        vx, vy, vz = np.where(flip, -vx, vx), np.where(flip, -vy, vy), np.where(flip, -vz, vz)
        if output_rot and rot_mat is not None:
            r = np.asarray(rot_mat).astype(T)[c]
            vx, vy, vz = (r[..., 0, 0] * vx + r[..., 0, 1] * vy + r[..., 0, 2] * vz,
                          r[..., 1, 0] * vx + r[..., 1, 1] * vy + r[..., 1, 2] * vz,
                          r[..., 2, 0] * vx + r[..., 2, 1] * vy + r[..., 2, 2] * vz)
    out[c] = np.stack([vx, vy, vz], axis=-1)
    return out


# ------------------------------------------------------------------------------------------------------------------
# pack_vertices
# ------------------------------------------------------------------------------------------------------------------
def vert_grid_len(num_vertices):
    """hz_vert_grid_len: 3 floats a vertex, 16 extra floats, plus what makes the byte size a multiple of 16"""
    nbytes = 3 * num_vertices * 4
    add = 16
    if nbytes % 16 != 0:
        add += (16 - nbytes % 16) // 4
    return 3 * num_vertices + add


def pack_vertices(x, y, z, length=None):
    """interleaved x, y, z followed by zeros up to `length` floats (default: vert_grid_len)"""
    n = x.size
    out = np.zeros(vert_grid_len(n) if length is None else length, np.float32)
    out[0:3 * n:3], out[1:3 * n:3], out[2:3 * n:3] = x.ravel(), y.ravel(), z.ravel()
    return out


# ------------------------------------------------------------------------------------------------------------------
# inputs shared by the CPU test of this module and the GPU test of the kernels
# ------------------------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 65537)                                  # around one workgroup of 256 lanes, and many blocks
LON_EDGES = (0.0, 90.0, -90.0, 180.0, -180.0, 270.0, 360.0)
LAT_EDGES = (0.0, 45.0, -45.0, 90.0, -90.0, 89.999999, -89.999999)
H_EDGES = (0.0, -430.0, 8848.0)


def geodetic_inputs(n, seed=0, lat_max=90.0):
    """n points: seeded random lon in [-180, 360), lat in [-lat_max, lat_max], h float32 in [-500, 9000]; where n has room
    for them, the last 49 are every pair of LON_EDGES x LAT_EDGES (latitudes clipped to lat_max) with H_EDGES in turn."""
    rng = np.random.default_rng(1000 * seed + n)
    lon = rng.uniform(-180.0, 360.0, n)
    lat = rng.uniform(-lat_max, lat_max, n)
    h = rng.uniform(-500.0, 9000.0, n).astype(np.float32)
    k = len(LON_EDGES) * len(LAT_EDGES)
    if n >= k:
        lo, la = np.meshgrid(LON_EDGES, LAT_EDGES)
        lon[n - k:], lat[n - k:] = lo.ravel(), np.clip(la.ravel(), -lat_max, lat_max)
        h[n - k:] = np.resize(np.array(H_EDGES, np.float32), k)
    return lon, lat, h


def patch_inputs(n, lon_or, lat_or, seed=0):
    """n points of the 1 degree x 1 degree patch around (lon_or, lat_or); every other longitude is written 360 degrees
    further east where the patch lies west of Greenwich (the same meridian, the other side of the antimeridian)"""
    rng = np.random.default_rng(2000 * seed + n)
    lon = rng.uniform(lon_or - 0.5, lon_or + 0.5, n)
    lat = rng.uniform(lat_or - 0.5, lat_or + 0.5, n)
    h = rng.uniform(-500.0, 9000.0, n).astype(np.float32)
    if lon_or < 0.0:
        lon[1::2] += 360.0
    if n >= 4:
        lon[-1], lat[-1], h[-1] = lon_or, lat_or, 0.0              # the origin itself: ENU (0, 0, 0) up to rounding
    return lon, lat, h


def swiss_inputs(n, seed=0):
    rng = np.random.default_rng(3000 * seed + n)
    lon = rng.uniform(5.9, 10.5, n)
    lat = rng.uniform(45.8, 47.8, n)
    h = rng.uniform(-500.0, 9000.0, n).astype(np.float32)
    if n >= 8:
        lon[-4:] = (5.9, 10.5, 5.9, 10.5)
        lat[-4:] = (45.8, 45.8, 47.8, 47.8)
        h[-4:] = (0.0, -430.0, 8848.0, 193.0)
    return lon, lat, h


def _terrain(rng, n0, n1, relief):
    """rough float32 terrain: a few random sinusoids plus noise, `relief` metres peak to peak at most"""
    i, j = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    z = np.zeros((n0, n1))
    for _ in range(6):
        a, b, p = rng.uniform(0.1, 0.6), rng.uniform(0.1, 0.6), rng.uniform(0.0, 6.28)
        z += rng.uniform(0.2, 1.0) * np.sin(a * i + b * j + p)
    z += 0.05 * rng.standard_normal((n0, n1))
    z = (z - z.min()) / (z.max() - z.min())
    return (100.0 + relief * z).astype(np.float32)


def _planar(n0, n1, dx, dy, ox=0.0, oy=0.0, y_up_with_row=False):
    xs = (ox + np.arange(n1) * dx).astype(np.float32)
    rows = np.arange(n0) if y_up_with_row else (n0 - 1 - np.arange(n0))
    ys = (oy + rows * dy).astype(np.float32)
    x, y = np.meshgrid(xs, ys)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def slope_arithmetic_grids():
    """{name: (x, y, z)} -- the 19 x 23 planar grids on which the float32 arithmetic of the slope kernels is judged"""
    rng = np.random.default_rng(7)
    n0, n1 = 19, 23
    g = {}
    x, y = _planar(n0, n1, 30.0, 30.0)
    g["rough_30m"] = (x, y, _terrain(rng, n0, n1, 800.0))
    x, y = _planar(n0, n1, 2.0, 2.0, 2.6e6, 1.2e6)
    g["swiss_2m"] = (x, y, _terrain(rng, n0, n1, 60.0))
    x, y = _planar(n0, n1, 1.0, 90.0)
    g["aspect_1x90"] = (x, y, _terrain(rng, n0, n1, 50.0))
    x, y = _planar(n0, n1, 30.0, 30.0)
    g["flat"] = (x, y, np.full((n0, n1), 250.0, np.float32))
    x, y = _planar(n0, n1, 30.0, 30.0, y_up_with_row=True)
    g["y_up_with_row"] = (x, y, _terrain(rng, n0, n1, 800.0))
    return g


BORDER_SHAPES = ((1, 1), (2, 7), (3, 3), (3, 258), (258, 3))


def slope_border_grid(n0, n1):
    rng = np.random.default_rng(100 * n0 + n1)
    x, y = _planar(n0, n1, 25.0, 25.0)
    return x, y, _terrain(rng, n0, n1, 400.0) if n0 * n1 > 1 else np.full((1, 1), 100.0, np.float32)


def slope_cases(gold):
    """(name, method, x, y, z, rot_mat, output_rot) of every grid on which tests/test_gpu_prep_reference.py judges the slope
    kernels; `gold` holds the arrays of tests/golden/prep_reference.npz (curved geometry, rot_mat with its NaN ring)"""
    fns = ("plane", "vector")
    for name, (x, y, z) in slope_arithmetic_grids().items():
        for meth in fns:
            yield name, meth, x, y, z, None, False
    for ellps in ELLPS_NAMES:
        k = ellps + "_"
        x, y, z, rot = gold[k + "x_enu"], gold[k + "y_enu"], gold[k + "z_enu"], gold[k + "rot"]
        for meth in fns:
            yield k + "enu", meth, x, y, z, None, False
            yield k + "enu+rot", meth, x, y, z, rot, False
            yield k + "enu+rot,output_rot", meth, x, y, z, rot, True
    for n0, n1 in BORDER_SHAPES:
        x, y, z = slope_border_grid(n0, n1)
        for meth in fns:
            yield "border_%dx%d" % (n0, n1), meth, x, y, z, None, False
