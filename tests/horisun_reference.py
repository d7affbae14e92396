"""DESIGN.md section 4, clause 10 in NumPy: shadow and sw_dir_cor from a stored horizon.

The float32 set-up is written with explicit np.float32 operations in the order of shadow_setup (hz_shadow.hip) -- NumPy
rounds every elementwise operation on its own, so there is no fused multiply-add to switch off -- and the look-up is float64
formed from the float32 values.  `lookup` returns, per (position, cell), the shadow code, sw_dir_cor and the margin
|alpha - h| of the terrain decision; `fold` is the clause 9 sum of per-position maps."""
import numpy as np

F = np.float32
TWO_PI = 6.283185307179586            # the double nearest to 2 pi (= 2 * np.pi)
MARGIN = 1.0e-9                       # [rad] decisions closer than this to the horizon are not held to the reference
CAP = 1.0e-4                          # at most this share of a case's unmasked (cell, position) pairs inside the margin


def dot_prod_min(ang_max):
    """cosf(deg2rad_f(ang_max)) of the library (shadow_comp.cpp:498): float in, double arithmetic, float out; cosf of the
    platform is within an ulp of np.cos rounded to float32 -- the tests use ang_max values where both agree."""
    rad = F((np.float64(F(ang_max)) / 180.0) * np.pi)
    return F(np.cos(np.float64(rad)))


def setup(sun, vert, vec_norm, vec_tilt):
    """float32: s = unit(p - o) with o = v + norm * 0.05f, dot_ns, dot_ts; sums associated (x + y) + z.
    sun f32[3]; vert, vec_norm, vec_tilt f32[..., 3].  Returns (s f32[..., 3], dot_ns, dot_ts)."""
    with np.errstate(all="ignore"):
        o = [vert[..., k] + vec_norm[..., k] * F(0.05) for k in range(3)]
        d = [F(sun[k]) - o[k] for k in range(3)]
        mag = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        s = [d[k] / mag for k in range(3)]
        dot_ns = (vec_norm[..., 0] * s[0] + vec_norm[..., 1] * s[1]) + vec_norm[..., 2] * s[2]
        dot_ts = (vec_tilt[..., 0] * s[0] + vec_tilt[..., 1] * s[1]) + vec_tilt[..., 2] * s[2]
    for a in s + [dot_ns, dot_ts]:
        assert a.dtype == np.float32
    return np.stack(s, axis=-1), dot_ns, dot_ts


def horizon_at(s, vec_norm, vec_north, hori):
    """float64 from float32 values: (h, alpha, k0, k1, t) of the look-up for sun directions s f32[..., 3] and horizon rows
    hori f32[..., A]."""
    A = hori.shape[-1]
    s64, n64, h64 = s.astype(np.float64), vec_norm.astype(np.float64), vec_north.astype(np.float64)
    with np.errstate(all="ignore"):
        ex = h64[..., 1] * n64[..., 2] - h64[..., 2] * n64[..., 1]
        ey = h64[..., 2] * n64[..., 0] - h64[..., 0] * n64[..., 2]
        ez = h64[..., 0] * n64[..., 1] - h64[..., 1] * n64[..., 0]
        cn = (s64[..., 0] * h64[..., 0] + s64[..., 1] * h64[..., 1]) + s64[..., 2] * h64[..., 2]
        ce = (s64[..., 0] * ex + s64[..., 1] * ey) + s64[..., 2] * ez
        cu = (s64[..., 0] * n64[..., 0] + s64[..., 1] * n64[..., 1]) + s64[..., 2] * n64[..., 2]
        phi = np.arctan2(ce, cn)
        phi = np.where(phi < 0.0, phi + TWO_PI, phi)
        u = phi * (np.float64(A) / TWO_PI)
        kf = np.minimum(np.maximum(np.floor(u), 0.0), np.float64(A))     # u is in [0, A]; NaN: 0
        kf = np.where(np.isnan(kf), 0.0, kf)
        t = u - kf
        k = kf.astype(np.int64)
        k0, k1 = k % A, (k + 1) % A
        h0 = np.take_along_axis(hori, k0[..., None], axis=-1)[..., 0].astype(np.float64)
        h1 = np.take_along_axis(hori, k1[..., None], axis=-1)[..., 0].astype(np.float64)
        h = (1.0 - t) * h0 + t * h1
        alpha = np.arcsin(np.minimum(np.maximum(cu, -1.0), 1.0))
    return h, alpha, k0, k1, t


def lookup(suns, hori, vert, vec_tilt, vec_norm, vec_north, surf_enl_fac, mask, fill, ang_max=89.0):
    """Per position s and cell: code u8[S][y][x] (0 lit, 1 self-shaded, 2 terrain-shaded, 3 masked), sw_dir_cor f32[S][y][x],
    margin f64[S][y][x] = |alpha - h| where the terrain decision was taken (inf elsewhere: masked, self-shaded, NaN horizon),
    and `alt`: what the two outputs would be had the terrain decision gone the other way (for pairs inside the margin).
    vert f32[y][x][3] = the vertices of the inner domain."""
    S = suns.shape[0]
    dpm = dot_prod_min(ang_max)
    code = np.empty((S,) + mask.shape, np.uint8)
    val = np.empty((S,) + mask.shape, np.float32)
    code_alt, val_alt = code.copy(), val.copy()
    margin = np.full((S,) + mask.shape, np.inf)
    for i in range(S):
        s, dot_ns, dot_ts = setup(suns[i], vert, vec_norm, vec_tilt)
        h, alpha, _, _, _ = horizon_at(s, vec_norm, vec_north, hori)
        with np.errstate(all="ignore"):
            shaded = alpha < h                          # NaN h: False
            lit_val = (dot_ts / np.maximum(dot_ns, dpm)) * surf_enl_fac
            assert lit_val.dtype == np.float32
            faces = dot_ts > F(0.0)
            inside = dot_ts > dpm
        for sh, c_out, v_out in ((shaded, code, val), (~shaded, code_alt, val_alt)):
            c_out[i] = np.where(faces, np.where(sh, 2, 0), 1)
            v_out[i] = np.where(inside & ~sh, lit_val, F(0.0))
            c_out[i][mask != 1] = 3
            v_out[i][mask != 1] = fill
        with np.errstate(all="ignore"):
            m = np.abs(alpha - h)
        margin[i] = np.where(faces & (mask == 1) & ~np.isnan(m), m, np.inf)
    return dict(code=code, val=val, margin=margin, code_alt=code_alt, val_alt=val_alt)


def fold(codes, vals, weights, mask, fill):
    """Clause 9: float64 accumulators, ascending s, acc += (double)w[s] * value, one rounding; masked cells get fill.
    Returns (sw_dir_cor_sum, sunlit_sum) f32[y][x]."""
    S = codes.shape[0]
    w = np.ones(S) if weights is None else weights.astype(np.float64)
    acc_sw, acc_lit = np.zeros(mask.shape), np.zeros(mask.shape)
    with np.errstate(all="ignore"):
        for i in range(S):
            acc_sw += w[i] * vals[i].astype(np.float64)
            acc_lit += w[i] * (codes[i] == 0)
        sw, lit = acc_sw.astype(np.float32), acc_lit.astype(np.float32)
    sw[mask != 1] = fill
    lit[mask != 1] = fill
    return sw, lit


# ---- the cases of tests/test_gpu_horisun.py (built here so that the CPU file can hold them to the exclusion cap) ----------

def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_case(dims, dem, offset, azim_num, num_sun, frame, seed, fill=np.nan, ang_max=89.0):
    """One seeded case: a DEM of `dem` vertices with gentle relief, an inner domain `dims` at `offset`, a random horizon in
    [-0.2, 0.9] rad, a planar or per-cell random orthonormal frame (north perpendicular to norm), unit tilts up to 60 degrees off
    norm, a mask with holes, and suns all round the compass at elevations from -20 to 90 degrees at 1.5e11."""
    rng = np.random.default_rng(seed)
    d0, d1 = dem
    n0, n1 = dims
    x = (np.arange(d1) * 30.0).astype(np.float32)
    y = ((d0 - 1 - np.arange(d0)) * 30.0).astype(np.float32)
    xx, yy = np.meshgrid(x, y)
    z = rng.uniform(100.0, 400.0, (d0, d1)).astype(np.float32)
    vert_grid = np.empty(d0 * d1 * 3 + 5, np.float32)             # (longer than needed: only `fits_grid` is asked)
    vert_grid[:] = 0.0
    vert_grid[0:3 * d0 * d1:3], vert_grid[1:3 * d0 * d1:3], vert_grid[2:3 * d0 * d1:3] = xx.ravel(), yy.ravel(), z.ravel()
    verts = vert_grid[:3 * d0 * d1].reshape(d0, d1, 3)
    vert = np.ascontiguousarray(verts[offset[0]:offset[0] + n0, offset[1]:offset[1] + n1])
    if frame == "planar":
        norm = np.zeros((n0, n1, 3)); norm[..., 2] = 1.0
        north = np.zeros((n0, n1, 3)); north[..., 1] = 1.0
    else:
        norm = unit(rng.standard_normal((n0, n1, 3)))
        r = rng.standard_normal((n0, n1, 3))
        north = unit(r - (r * norm).sum(-1, keepdims=True) * norm)
    east = np.cross(north, norm)
    off = np.deg2rad(60.0) * rng.random((n0, n1, 1))
    dirn = rng.uniform(0.0, 2.0 * np.pi, (n0, n1, 1))
    tilt = np.cos(off) * norm + np.sin(off) * (np.cos(dirn) * north + np.sin(dirn) * east)
    vec_norm, vec_north, vec_tilt = (np.ascontiguousarray(v, np.float32) for v in (norm, north, tilt))
    enl = rng.uniform(1.0, 1.6, (n0, n1)).astype(np.float32)
    mask = (rng.random((n0, n1)) > 0.15).astype(np.uint8)
    if n0 * n1 > 1:
        mask.flat[0] = 0
        mask.flat[-1] = 1
    else:
        mask[:] = 1
    hori = rng.uniform(-0.2, 0.9, (n0, n1, azim_num)).astype(np.float32)
    # suns in the planar frame's compass (east = x, north = y, up = z), about the domain's centre cell
    ci, cj = n0 // 2, n1 // 2
    centre = vert[ci, cj].astype(np.float64)
    az = rng.uniform(0.0, 2.0 * np.pi, num_sun)
    el = np.deg2rad(rng.uniform(-20.0, 90.0, num_sun))
    d = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)
    suns = (centre[None, :] + 1.5e11 * d).astype(np.float32)
    if num_sun >= 5:
        e = np.deg2rad(35.0)
        # exactly due north of the centre cell's column: sun_x = that column's x, so ce = 0 and cn > 0 there (planar frame)
        suns[-1] = (vert[ci, cj, 0], F(1.5e11 * np.cos(e)), F(1.5e11 * np.sin(e)))
        # a hair west of north: the wrap from k0 = A - 1 to k1 = 0
        suns[-2] = (F(-1.5e11 * np.cos(e) * 1.0e-6), F(1.5e11 * np.cos(e)), F(1.5e11 * np.sin(e)))
        # the zenith of the centre cell: cn = ce = 0 there (planar frame)
        suns[-3] = (vert[ci, cj, 0], vert[ci, cj, 1], F(1.5e11))
    return dict(azim_num=azim_num, hori=hori, vert_grid=vert_grid, dem_dim_0=d0, dem_dim_1=d1, offset_0=offset[0],
                offset_1=offset[1], vert=vert, vec_tilt=vec_tilt, vec_norm=vec_norm, vec_north=vec_north, surf_enl_fac=enl,
                mask=mask, suns=suns, fill=fill, ang_max=ang_max)


CHUNK_TEST = 3          # hz_debug_set("horisun_chunk", 3) in the GPU file: S = 5 is then "larger than the position chunk"

# (name, dims, dem, offset, azim_num, num_sun, frame, seed): every grid, A in {1, 2, 7, 360}, S in {1, 5}, both frames
CASES = [
    ("inner_A360_planar", (37, 53), (45, 61), (4, 4), 360, 5, "planar", 101),
    ("inner_A7_random", (37, 53), (45, 61), (4, 4), 7, 5, "random", 102),
    ("inner_A2_random", (37, 53), (45, 61), (3, 5), 2, 5, "random", 103),
    ("inner_A1_planar", (37, 53), (45, 61), (8, 0), 1, 1, "planar", 104),
    ("cell_A360_random", (1, 1), (3, 3), (1, 1), 360, 5, "random", 105),
    ("cell_A1_planar", (1, 1), (1, 1), (0, 0), 1, 1, "planar", 106),
    ("row_A7_planar", (1, 130), (1, 130), (0, 0), 7, 5, "planar", 107),
    ("row_A360_random", (1, 130), (3, 134), (1, 2), 360, 1, "random", 108),
    ("row_A2_planar", (1, 130), (2, 131), (1, 1), 2, 5, "planar", 109),
]


def case(name):
    for c in CASES:
        if c[0] == name:
            return make_case(*c[1:])
    raise KeyError(name)


def reference(c):
    return lookup(c["suns"], c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"],
                  c["mask"], c["fill"], c["ang_max"])


def inside_margin_share(c, ref):
    """Share of the unmasked (cell, position) pairs of a case whose terrain decision lies inside the margin."""
    unmasked = int((c["mask"] == 1).sum()) * c["suns"].shape[0]
    return float((ref["margin"] <= MARGIN).sum()) / max(unmasked, 1)
