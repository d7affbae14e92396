"""ctypes front end of oracle/_ref/libhz_ref.so: the reference's OWN horizon_comp.cpp / shadow_comp.cpp, compiled
unmodified (oracle/Makefile, ``make ref``) and linked with a stand-in Embree that answers every ray with the oracle's
scene and triangle test (oracle/ref/standin.cpp).

TEST INFRASTRUCTURE ONLY.  Same call shapes as ``oracle.oracle`` (``horizon_gridded``, ``horizon_locations``,
``Terrain``), so a test runs one input through both and compares bit patterns: the reference's statements, executed,
against the oracle's restatement of them.  The library exists only where ``build()`` found the reference tree, or where
it was carried along; ``available()`` says which.

The reference prints its progress to stdout; that is captured at file-descriptor level around each call and the
"Number of rays shot" line is returned as a statistic next to the stand-in's own count.

Ray budget: ray_guess_const / ray_discrete_sampling of the reference do not return when a ray is still blocked at the
top table index or still free at index 0 (the oracle's "guard events").  Every call here runs under a budget of rays
(``max_rays``; default: generous multiple of the table size per azimuth); exceeding it raises ``RayBudgetExceeded``
instead of hanging the caller.
"""
import ctypes as C
import os
import re
import tempfile

import numpy as np

from . import oracle as _orc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libhz_ref.so")
_lib = None


class RayBudgetExceeded(RuntimeError):
    """The reference's search did not end within the ray budget (a guard case of the oracle)."""


class StandinError(RuntimeError):
    """The stand-in Embree refused what the reference asked of it (topology check, unmodelled query)."""


def available():
    return os.path.exists(LIB_PATH)


def reference_dir():
    """Root of the reference tree ``make ref`` compiles from: $HZ_REFERENCE, else the default of oracle/Makefile."""
    env = os.environ.get("HZ_REFERENCE")
    if env:
        return env
    with open(os.path.join(_HERE, "Makefile")) as f:
        return re.search(r"^HZ_REFERENCE \?= (\S+)", f.read(), re.M).group(1)


def reference_present():
    d = os.path.join(reference_dir(), "horayzon")
    return all(os.path.isfile(os.path.join(d, n)) for n in
               ("horizon_comp.cpp", "horizon_comp.h", "shadow_comp.cpp", "shadow_comp.h"))


def build():
    """``make ref`` where the reference tree is present; elsewhere whatever oracle/_ref/ holds is left as it is."""
    import subprocess
    if reference_present():
        subprocess.check_call(["make", "-s", "-C", _HERE, "HZ_REFERENCE=" + reference_dir(), "ref"])
    return LIB_PATH if available() else None


def lib():
    global _lib
    if _lib is None:
        _orc.lib()      # the oracle first, by path: libhz_ref.so binds to this instance (its flags are shared)
        L = C.CDLL(LIB_PATH)
        fp, u8p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        L.hzref_last_error.restype = C.c_char_p
        L.hzref_set_ray_budget.argtypes = [C.c_int64]
        L.hzref_rays_cast.restype = C.c_int64
        L.hzref_set_mode.argtypes = [C.c_int]
        L.hzref_record.argtypes = [fp, C.c_int64]
        L.hzref_recorded.restype = C.c_int64
        L.hzref_horizon_gridded.restype = C.c_int
        L.hzref_horizon_gridded.argtypes = [
            fp, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
            C.c_char_p, C.c_char_p, fp, C.c_int, i32p, C.c_int, C.c_float, u8p, C.c_float, C.c_float]
        L.hzref_horizon_locations.restype = C.c_int
        L.hzref_horizon_locations.argtypes = [
            fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_char_p, C.c_char_p,
            C.c_float, fp, C.c_int]
        L.hzref_terrain_new.restype = C.c_void_p
        L.hzref_terrain_initialise.restype = C.c_int
        L.hzref_terrain_initialise.argtypes = [
            C.c_void_p, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, fp, fp, u8p, C.c_char_p,
            C.c_float, C.c_float, C.c_int]
        L.hzref_terrain_shadow.restype = C.c_int
        L.hzref_terrain_shadow.argtypes = [C.c_void_p, fp, u8p]
        L.hzref_terrain_sw_dir_cor.restype = C.c_int
        L.hzref_terrain_sw_dir_cor.argtypes = [C.c_void_p, fp, fp]
        L.hzref_terrain_delete.argtypes = [C.c_void_p]
        _lib = L
    return _lib


_f, _u8, _i32 = _orc._f, _orc._u8, _orc._i32
last_stdout = ""        # what the reference printed during the most recent call


class _Captured:
    """Run a block with file descriptor 1 pointing at a temporary file (the reference writes through both printf and
    std::cout); ``text`` holds what was written."""

    def __enter__(self):
        import sys
        sys.stdout.flush()
        self._tmp = tempfile.TemporaryFile(mode="w+b")
        self._saved = os.dup(1)
        os.dup2(self._tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        global last_stdout
        C.CDLL(None).fflush(None)
        os.dup2(self._saved, 1)
        os.close(self._saved)
        self._tmp.seek(0)
        self.text = last_stdout = self._tmp.read().decode("utf-8", "replace")
        self._tmp.close()
        return False


def _call(fn, args, max_rays, record=None):
    """One guarded call: budget, stdout capture, optional ray recording, error translation.  Returns (what the reference
    printed, rays the stand-in counted, the recorded rays or None)."""
    L = lib()
    rec = None
    if record:
        rec = np.zeros((int(record), 8), np.float32)
        L.hzref_record(_f(rec), int(record))
    L.hzref_set_ray_budget(int(max_rays))
    try:
        with _Captured() as cap:
            rc = fn(*args)
    finally:
        n_rec = int(L.hzref_recorded())
        L.hzref_record(None, 0)
    rays = int(L.hzref_rays_cast())
    L.hzref_set_ray_budget(-1)
    if rc == 1:
        raise RayBudgetExceeded("the reference did not finish within %d rays" % max_rays)
    if rc == 2:
        raise StandinError(L.hzref_last_error().decode())
    if rc != 0:
        raise ValueError("invalid argument for the reference (code %d)" % rc)
    return cap.text, rays, (rec[:n_rec] if rec is not None else None)


def _printed_rays(text):
    m = re.search(r"Number of rays shot: (\d+)", text)
    return int(m.group(1)) if m else None


def set_mode(mode=_orc.MODE_BVH):
    """How the stand-in queries the oracle's scene: MODE_BVH (default) or MODE_BRUTE."""
    lib().hzref_set_mode(int(mode))


def _default_budget(cells, azim_num, hori_acc, elev_ang_low_lim):
    # a search that ends never casts more than one ray per table entry and azimuth (the table has
    # ~ 5 (89.98 - low) / hori_acc entries); twice that, plus the two surface rays of a location
    per_azim = 2.0 * (5.0 * (90.0 - elev_ang_low_lim) / hori_acc + 2.0)
    return int(cells * (azim_num * per_azim + 2)) + 16


def horizon_gridded(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north, offset_0, offset_1, dist_search,
                    azim_num=360, hori_acc=0.25, ray_algorithm="guess_constant", geom_type="grid", vert_simp=None,
                    num_vert_simp=1, tri_ind_simp=None, num_tri_simp=1, elev_ang_low_lim=-15.0, mask=None,
                    hori_fill=0.0, ray_org_elev=0.01, *, max_rays=None, record=None, return_stats=False):
    """The reference's horizon_gridded_comp (horizon_comp.cpp:629-822) on the oracle's intersector.  Returns
    (hori, azim) like oracle.horizon_gridded; with ``return_stats`` also dict(rays=<printed by the reference>,
    rays_cast=<counted by the stand-in>, recorded=<(n, 8) rays if ``record``>)."""
    if vert_simp is None:
        vert_simp = np.zeros(4, np.float32)
    if tri_ind_simp is None:
        tri_ind_simp = np.zeros(4, np.int32)
    vert_grid = np.ascontiguousarray(vert_grid, np.float32)
    vec_norm = np.ascontiguousarray(vec_norm, np.float32)
    vec_north = np.ascontiguousarray(vec_north, np.float32)
    vert_simp = np.ascontiguousarray(vert_simp, np.float32)
    tri_ind_simp = np.ascontiguousarray(tri_ind_simp, np.int32)
    d0, d1 = vec_norm.shape[:2]
    if mask is None:
        mask = np.ones((d0, d1), np.uint8)
    mask = np.ascontiguousarray(mask, np.uint8)
    hori = np.full((d0, d1, azim_num), np.nan, np.float32)
    if max_rays is None:
        max_rays = _default_budget(d0 * d1, azim_num, hori_acc, elev_ang_low_lim)
    text, rays, rec = _call(lib().hzref_horizon_gridded, (
        _f(vert_grid), dem_dim_0, dem_dim_1, _f(vec_norm), _f(vec_north), offset_0, offset_1, _f(hori), d0, d1,
        azim_num, dist_search, hori_acc, ray_algorithm.encode(), geom_type.encode(), _f(vert_simp), num_vert_simp,
        _i32(tri_ind_simp), num_tri_simp, elev_ang_low_lim, _u8(mask), hori_fill, ray_org_elev), max_rays, record)
    azim = np.empty(azim_num, np.float32)
    for i in range(azim_num):
        azim[i] = ((2 * np.pi) / azim_num * i)
    if return_stats:
        return hori, azim, dict(rays=_printed_rays(text), rays_cast=rays, recorded=rec)
    return hori, azim


def horizon_locations(vert_grid, dem_dim_0, dem_dim_1, coords, vec_norm, vec_north, dist_search, azim_num=360,
                      hori_acc=0.25, ray_algorithm="binary_search", geom_type="grid", elev_ang_low_lim=-89.98,
                      ray_org_elev=np.array([0.01], dtype=np.float32), hori_dist_out=False, *, max_rays=None,
                      record=None, return_stats=False):
    """The reference's horizon_locations_comp (horizon_comp.cpp:828-1094) on the oracle's intersector.  ``rays`` is the
    count the reference prints (search rays; its two surface rays per location are not in it), ``rays_cast`` what the
    stand-in saw (both)."""
    vert_grid = np.ascontiguousarray(vert_grid, np.float32)
    coords = np.ascontiguousarray(coords, np.float32)
    vec_norm = np.ascontiguousarray(vec_norm, np.float32)
    vec_north = np.ascontiguousarray(vec_north, np.float32)
    n = coords.shape[0]
    roe = np.ascontiguousarray(ray_org_elev, np.float32)
    if len(roe) != n:
        roe = np.repeat(roe, n)
    if hori_dist_out and ray_algorithm == "guess_constant":
        raise TypeError("horizon detection algorithm 'guess_constant' not implemented for horizon "
                        "distance computation")
    hori = np.full((n, azim_num), np.nan, np.float32)
    dist = np.full((n if hori_dist_out else 1, azim_num), np.nan, np.float32)
    if max_rays is None:
        max_rays = _default_budget(n, azim_num, hori_acc, elev_ang_low_lim)
    text, rays, rec = _call(lib().hzref_horizon_locations, (
        _f(vert_grid), dem_dim_0, dem_dim_1, _f(coords), _f(vec_norm), _f(vec_north), _f(hori), _f(dist), n, azim_num,
        dist_search, hori_acc, ray_algorithm.encode(), geom_type.encode(), elev_ang_low_lim, _f(roe),
        int(bool(hori_dist_out))), max_rays, record)
    azim = np.empty(azim_num, np.float32)
    for i in range(azim_num):
        azim[i] = ((2 * np.pi) / azim_num * i)
    out = (hori, dist, azim) if hori_dist_out else (hori, azim)
    if return_stats:
        return out + (dict(rays=_printed_rays(text), rays_cast=rays, recorded=rec),)
    return out


class Terrain:
    """The reference's shapes::CppTerrain (shadow_comp.cpp:304-605) on the oracle's intersector; call shapes of
    oracle.Terrain.  ``rays`` is the stand-in's count for the most recent call (at most one ray per cell)."""

    def __init__(self):
        self._h = lib().hzref_terrain_new()
        if not self._h:
            raise StandinError(lib().hzref_last_error().decode())
        self._keep = None
        self.rays = 0

    def initialise(self, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1, vec_tilt, vec_norm, surf_enl_fac,
                   elevation, mask, geom_type="grid", sw_dir_cor_fill=np.nan, ang_max=89.0, refrac_cor=False):
        in0, in1 = vec_tilt.shape[:2]
        a = [np.array(x, np.float32, order="C") for x in (vert_grid, vec_tilt, vec_norm, surf_enl_fac, elevation)]
        m = np.array(mask, np.uint8, order="C")
        self._keep = (a, m)            # the reference keeps the pointers, not copies (shadow_comp.cpp:332-346)
        self._cells = in0 * in1
        _call(lib().hzref_terrain_initialise, (
            self._h, _f(a[0]), dem_dim_0, dem_dim_1, offset_0, offset_1, _f(a[1]), _f(a[2]), in0, in1, _f(a[3]),
            _f(a[4]), _u8(m), geom_type.encode(), sw_dir_cor_fill, ang_max, int(refrac_cor)), 0)

    def shadow(self, sun_position, shadow_buffer):
        sp = np.ascontiguousarray(sun_position, np.float32)
        _, self.rays, _ = _call(lib().hzref_terrain_shadow, (self._h, _f(sp), _u8(shadow_buffer)), self._cells)

    def sw_dir_cor(self, sun_position, sw_dir_cor_buffer):
        sp = np.ascontiguousarray(sun_position, np.float32)
        _, self.rays, _ = _call(lib().hzref_terrain_sw_dir_cor, (self._h, _f(sp), _f(sw_dir_cor_buffer)), self._cells)

    def __del__(self):
        if getattr(self, "_h", None):
            lib().hzref_terrain_delete(self._h)
            self._h = None
