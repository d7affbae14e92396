"""horayzon.horizon -- terrain horizon on MI355X.

Host-side mirror of the reference's Cython boundary ``horayzon/horizon.pyx``:
same function name, positional order, defaults, validation order and
exception classes (horizon.pyx:29-49, 109-156); the computation runs in
hand-written HIP kernels behind the C ABI (hz_horizon_gridded).
"""
import ctypes as C

import numpy as np

from . import _lib
from . import _validate as V
from ._lib import Scene, hz_opts, hz_stats, hz_topo_out, ptr

TOPO_NAMES = ("svf", "vsf", "openness")     # the reductions `topo=` can ask for (hz_opts.svf, hz_topo_out.vsf / .openness)
LAYOUTS = ("cell_major", "azim_major")      # hori (y, x, azim) as the reference has it, or planes (azim, y, x)
HORI_DTYPES = ("float32", "uint16")         # the horizon as float32 [radian] or as the 16-bit code of `quantise`
# the 16-bit horizon code (clause 15): 65535 levels over [-pi/2, pi/2] and one code for NaN
Q16_NAN = 0xFFFF
Q16_STEP = 1.5707963267948966 / 32767.0     # [radian] between two codes
Q16_MAX_ERROR = Q16_STEP / 2 + 2 ** -24     # of decode(encode(v)) for v in range: half a step and half a float32 ulp below 2 rad
last_stats = None   # hz_stats of the most recent call as a dict (timers, ray count)
# test hook: defaults of the launch-schedule options ("left_min", "persist_grid", "left_cap_test": hz_opts) for calls that do not
# pass them -- lets the parity tests run their cases under other schedules without touching every call
schedule_overrides = {}


def _check_f32(a, ndim, name):
    # Cython's typed-buffer arguments raise ValueError on dtype/ndim mismatch
    if not isinstance(a, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)"
                        % (name, type(a).__name__))
    if a.ndim != ndim:
        raise ValueError("Buffer has wrong number of dimensions (expected %d, got %d)" % (ndim, a.ndim))
    if a.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t' but got '%s'" % a.dtype.name)


def check_layout(layout):
    """``layout=`` of the functions that write or read a horizon: one of ``LAYOUTS``."""
    if not isinstance(layout, str) or layout not in LAYOUTS:
        raise ValueError("unknown 'layout': %r (choose from %r)" % (layout, LAYOUTS))
    return layout == "azim_major"


def _convert(hori, to_planes, device):
    name = "hori" if to_planes else "planes"
    tensor = not isinstance(hori, np.ndarray) and hasattr(hori, "data_ptr")
    if not isinstance(hori, np.ndarray) and not tensor:
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray or torch.Tensor, got %s)"
                        % (name, type(hori).__name__))
    ndim = hori.dim() if tensor else hori.ndim
    if ndim != 3:
        raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % ndim)
    if str(hori.dtype).split(".")[-1] != "float32":
        raise ValueError("Buffer dtype mismatch, expected 'float32_t' but got '%s'" % str(hori.dtype).split(".")[-1])
    if min(hori.shape) < 1:
        raise ValueError("Inconsistent/incorrect shape of '%s'" % name)
    if not (hori.is_contiguous() if tensor else hori.flags["C_CONTIGUOUS"]):
        raise ValueError("array '%s' is not C-contiguous" % name)
    if to_planes:
        (y, x, a), shape = hori.shape, (hori.shape[2], hori.shape[0], hori.shape[1])
    else:
        (a, y, x), shape = hori.shape, (hori.shape[1], hori.shape[2], hori.shape[0])
    if tensor:
        import torch
        if hori.device.type != "cuda":
            raise ValueError("tensor '%s' is not on a GPU" % name)
        device = hori.device.index
        out = torch.empty(shape, dtype=torch.float32, device=hori.device)
        torch.cuda.synchronize(hori.device)       # the library works on a stream of its own
    else:
        out = np.empty(shape, dtype=np.float32)
    L = _lib.lib()
    _lib.check((L.hz_hori_to_planes if to_planes else L.hz_hori_from_planes)(ptr(hori), y, x, a, ptr(out), device))
    return out


def to_azim_major(hori, *, device=0):
    """``hori`` float32 (y, x, azim) -> planes float32 (azim, y, x), transposed on the GPU word for word (NaN payloads
    included).  A NumPy array gives a NumPy array (staged through the GPU ``device`` in bounded chunks); a torch tensor on a
    GPU gives a torch tensor on that GPU.  The input must be C-contiguous."""
    return _convert(hori, True, device)


def to_cell_major(planes, *, device=0):
    """The inverse of ``to_azim_major``: planes float32 (azim, y, x) -> ``hori`` float32 (y, x, azim)."""
    return _convert(planes, False, device)


def _q16_tensor_dtype():
    import torch
    return getattr(torch, "uint16", torch.int16)      # (older torch: int16 carries the same bits)


def _q16_convert(a, encode, device):
    name = "hori" if encode else "q"
    tensor = not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")
    if not isinstance(a, np.ndarray) and not tensor:
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray or torch.Tensor, got %s)"
                        % (name, type(a).__name__))
    dtype = str(a.dtype).split(".")[-1]
    accepted = ("float32",) if encode else (("uint16", "int16") if tensor else ("uint16",))
    if dtype not in accepted:
        raise ValueError("Buffer dtype mismatch, expected '%s_t' but got '%s'" % (accepted[0], dtype))
    if not (a.is_contiguous() if tensor else a.flags["C_CONTIGUOUS"]):
        raise ValueError("array '%s' is not C-contiguous" % name)
    shape = tuple(a.shape)
    if tensor:
        import torch
        if a.device.type != "cuda":
            raise ValueError("tensor '%s' is not on a GPU" % name)
        device = a.device.index
        out = torch.empty(shape, dtype=_q16_tensor_dtype() if encode else torch.float32, device=a.device)
        torch.cuda.synchronize(a.device)          # the library works on a stream of its own
        n = a.numel()
    else:
        out = np.empty(shape, dtype=np.uint16 if encode else np.float32)
        n = a.size
    L = _lib.lib()
    _lib.check((L.hz_hori_quantise if encode else L.hz_hori_dequantise)(ptr(a), n, ptr(out), device))
    return out


def quantise(hori, *, device=0):
    """``hori`` float32 [radian], any shape -> the 16-bit horizon code, uint16 of the same shape, encoded on the GPU
    (clause 15): ``rint`` of the angle, clamped to [-pi/2, pi/2], in steps of ``Q16_STEP`` = 0.0027
    degrees, plus 32767; NaN becomes ``Q16_NAN``.  ``dequantise(quantise(v))`` is within ``Q16_MAX_ERROR`` of every ``v`` in
    range.  A NumPy array gives a NumPy array (staged through the GPU ``device`` in bounded chunks); a torch tensor on a GPU
    gives a torch tensor on that GPU (``torch.uint16``, or ``torch.int16`` with the same bits where torch has no uint16).
    The input must be C-contiguous.  The code is elementwise: it is the same for both horizon layouts."""
    return _q16_convert(hori, True, device)


def dequantise(q, *, device=0):
    """The decoder of ``quantise``: codes uint16 (for a tensor also int16 carrying the same bits), any shape -> float32
    [radian]; ``Q16_NAN`` gives NaN.  ``quantise(dequantise(q)) == q`` for every code."""
    return _q16_convert(q, False, device)


def _hori_kind(planes, q16):
    return (_lib.HORI_PLANES if planes else 0) | (_lib.HORI_U16 if q16 else 0)


def horizon_gridded(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north,
                    offset_0, offset_1, dist_search, azim_num=360, hori_acc=0.25,
                    ray_algorithm="guess_constant", geom_type="grid",
                    vert_simp=np.array([0.0, 0.0, 0.0, 0.0], dtype=np.float32),
                    num_vert_simp=1,
                    tri_ind_simp=np.array([0, 0, 0, 0], dtype=np.int32),
                    num_tri_simp=1, elev_ang_low_lim=-15.0, mask=None,
                    hori_fill=0.0, ray_org_elev=0.01, *, device=0, verbose=False,
                    scene=None, svf_vec_tilt=None, svf_only=False, rows=None, count_work=False, devices=None,
                    topo=None, topo_vec_tilt=None, topo_only=False, layout="cell_major", hori_dtype="float32",
                    hori_dist=False, _top_nodes=-1, _regroup=-1, _hit_cache=True, _chunk_rows=0, _near_skip=True, _level_stack=False,
                    _verify_near=False, _left_min=0, _persist_grid=0, _verbose=0):
    """Horizon computation for gridded domain.

    Parameters, units and return values are those of the reference
    (horizon.pyx:50-106): ``hori_buffer`` float32 (y, x, azim_num) [radian],
    ``azim`` float32 (azim_num) [radian].

    Additional keyword-only arguments (not in the reference): ``device`` (HIP
    ordinal), ``verbose`` (print the reference's stdout report), ``scene`` (a
    prebuilt ``Scene`` to skip the BVH build), ``svf_vec_tilt`` (tilted normals;
    when given the sky view factor is accumulated in the same kernel and
    returned as a third value; with ``svf_only`` the horizon array is never materialised --
    it lives in a bounded device buffer, chunk by chunk -- and ``None`` is returned in its place:
    the 14401^2 mosaic would need 298 GB of horizon), ``rows`` ((begin, end) slab of inner-domain rows
    to compute; the rest of ``hori_buffer`` stays NaN), ``count_work``, ``devices``
    ("all" or a sequence of HIP ordinals: the inner-domain rows are split into one slab per
    entry, balanced by ``mask``, and each slab is computed by its own host thread on its own
    GPU -- the scene is built per device, nothing is exchanged, every thread copies its rows
    straight into the returned array; the multi-process form of the same sharding is
    ``horayzon_amd.dist``), ``topo`` (names from ``TOPO_NAMES``: the sky view factor, visible sky
    fraction and positive topographic openness are reduced from the horizon in the same call, one
    launch per horizon chunk, and returned as a third value ``{name: float32 (y, x)}``; "svf" and
    "vsf" need ``topo_vec_tilt``, the tilted normals; with ``topo_only`` the horizon is never
    materialised and ``None`` is returned in its place; each map is bit-identical to the
    ``topo_param`` function applied to the returned horizon), ``layout`` ("cell_major": the reference's
    (y, x, azim_num); "azim_major": the returned horizon is float32 (azim_num, y, x), the planes
    ``to_azim_major`` makes of the cell-major result, word for word -- the layout ``HorizonTerrain`` reads
    fastest; the cell-major array is never materialised, every other argument keeps its meaning, and
    ``svf_only`` / ``topo_only`` are refused: there is nothing to lay out), ``hori_dtype`` ("float32"; "uint16": the returned
    horizon is ``quantise`` of the float32 horizon of the same ``layout``, word for word, at half the bytes in memory and
    over the bus -- each chunk of rows is encoded on the GPU after it was traced and reduced, so the maps of ``topo`` /
    ``svf_vec_tilt`` are those of the float32 call; with ``rows`` the rest of the array is ``Q16_NAN``; ``svf_only`` /
    ``topo_only`` are refused), ``hori_dist`` (True: the distance to the horizon [metre] is computed in the same call and
    returned as second value -- ``(hori, dist, azim)``, the order of ``horizon_locations``, or ``(hori, dist, azim, third)``
    where a third value is returned -- float32 in ``layout``; it is ``horizon_distance`` of the float32 horizon of this call,
    word for word, also with ``hori_dtype="uint16"``: each chunk of rows gets its distances on the GPU before it is laid out
    or encoded; the horizon and the maps are those of the call without it; with ``rows`` the rest is NaN; ``svf_only`` /
    ``topo_only`` are refused).
    """
    global last_stats
    _check_f32(vert_grid, 1, "vert_grid")
    _check_f32(vec_norm, 3, "vec_norm")
    _check_f32(vec_north, 3, "vec_north")
    _check_f32(vert_simp, 1, "vert_simp")
    if not isinstance(tri_ind_simp, np.ndarray) or tri_ind_simp.ndim != 1 or tri_ind_simp.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int32_t' for tri_ind_simp")
    if mask is not None and (not isinstance(mask, np.ndarray) or mask.ndim != 2):
        raise ValueError("Buffer has wrong number of dimensions (expected 2) for mask")

    # Consistency and validity of the arguments: the reference's checks, classes, messages and order (horizon.pyx:109-153)
    if mask is None:
        mask = np.ones(vec_norm.shape[:2], dtype=np.uint8)
    V.run((
        (ValueError, "inconsistency between input arguments vert_grid, dem_dim_0 and dem_dim_1",
         lambda: not V.fits_grid(len(vert_grid), dem_dim_0, dem_dim_1)),
        (ValueError, "inconsistency between input arguments dem_dim_0, dem_dim_1, offset_0, offset_1 and vec_norm",
         lambda: not V.window_inside(offset_0, offset_1, vec_norm.shape, dem_dim_0, dem_dim_1)),
        (ValueError, V.MSG_NORTH, lambda: not V.same_leading_shape((vec_norm, vec_north), 3, 3)),
        (ValueError, V.MSG_ALG, lambda: ray_algorithm not in V.ALGORITHMS),
        (ValueError, V.MSG_GEOM, lambda: geom_type not in V.GEOMETRIES),
        (ValueError, "inconsistency between input arguments vert_simp and num_vert_simp", lambda: len(vert_simp) < num_vert_simp * 3),
        (ValueError, "inconsistency between input arguments tri_ind_simp and num_tri_simp", lambda: len(tri_ind_simp) < num_tri_simp * 3),
        (ValueError, "triangle indices of simplified outer domain exceed number of vertices",
         lambda: tri_ind_simp.max() > num_vert_simp - 1),
        (ValueError, V.MSG_ACC, lambda: hori_acc > 10.0),
        (ValueError, "shape of mask is inconsistent with other input", lambda: mask.shape[:2] != vec_norm.shape[:2]),
        (TypeError, V.MSG_MASK_TYPE, lambda: mask.dtype != "uint8"),
        (TypeError, V.MSG_ELEV, lambda: ray_org_elev < 0.005),
        (ValueError, V.MSG_DIM_LIMIT, lambda: max(dem_dim_0, dem_dim_1) > V.DIM_LIMIT),
        (ValueError, "vertex buffer vert_simp is larger than 16 GB", lambda: vert_simp.nbytes > 16.0e9),
    ))

    # further reductions in the same call (not in the reference): checked before anything reaches the library
    names = None if topo is None else ([topo] if isinstance(topo, str) else list(topo))
    tilted = names is not None and ("svf" in names or "vsf" in names)
    if topo_vec_tilt is not None:
        _check_f32(topo_vec_tilt, 3, "topo_vec_tilt")
    V.run((
        (ValueError, "'topo_only' needs 'topo'", lambda: topo_only and names is None),
        (ValueError, "'topo' cannot be combined with 'svf_vec_tilt' or 'svf_only' (ask for \"svf\" in 'topo')",
         lambda: names is not None and (svf_vec_tilt is not None or svf_only)),
        (ValueError, "'topo' is empty", lambda: names is not None and not names),
        (ValueError, "unknown name(s) in 'topo': %r (choose from %r)" % (
            [n for n in (names or ()) if n not in TOPO_NAMES], TOPO_NAMES),
         lambda: any(n not in TOPO_NAMES for n in names or ())),
        (ValueError, "'svf' and 'vsf' in 'topo' need 'topo_vec_tilt'", lambda: tilted and topo_vec_tilt is None),
        (ValueError, "'svf' and 'vsf' in 'topo' need azim_num >= 2", lambda: tilted and azim_num < 2),
        (ValueError, "shape of topo_vec_tilt is inconsistent with vec_norm",
         lambda: topo_vec_tilt is not None and topo_vec_tilt.shape != vec_norm.shape),
    ))

    planes = check_layout(layout)
    if planes and (svf_only or topo_only):
        raise ValueError("'svf_only' / 'topo_only' cannot be combined with layout=\"azim_major\": there is no horizon to lay out")
    if not isinstance(hori_dtype, str) or hori_dtype not in HORI_DTYPES:
        raise ValueError("unknown 'hori_dtype': %r (choose from %r)" % (hori_dtype, HORI_DTYPES))
    q16 = hori_dtype == "uint16"
    if q16 and (svf_only or topo_only):
        raise ValueError("'svf_only' / 'topo_only' cannot be combined with hori_dtype=\"uint16\": there is no horizon to encode")
    if hori_dist and (svf_only or topo_only):
        raise ValueError("'svf_only' / 'topo_only' cannot be combined with 'hori_dist': there is no horizon to return it with")

    # Ensure that passed arrays are contiguous in memory (horizon.pyx:159-163)
    vert_grid = np.ascontiguousarray(vert_grid)
    vec_norm = np.ascontiguousarray(vec_norm)
    vec_north = np.ascontiguousarray(vec_north)
    vert_simp = np.ascontiguousarray(vert_simp)
    tri_ind_simp = np.ascontiguousarray(tri_ind_simp)
    mask = np.ascontiguousarray(mask)

    dim_in_0, dim_in_1 = vec_norm.shape[0], vec_norm.shape[1]
    # Allocate horizon array (horizon.pyx:170-173)
    if svf_only and svf_vec_tilt is None:
        raise ValueError("'svf_only' needs 'svf_vec_tilt'")
    hori_shape = (azim_num, dim_in_0, dim_in_1) if planes else (dim_in_0, dim_in_1, azim_num)
    hori_buffer = None if (svf_only or topo_only) else np.empty(hori_shape, dtype=np.uint16 if q16 else np.float32)
    if rows is not None and hori_buffer is not None:
        hori_buffer.fill(Q16_NAN if q16 else np.nan)   # only a slab is written; every cell is written otherwise
                                   # (masked ones get hori_fill), so the 18 GB pre-fill is skipped
    dist_buffer = np.empty(hori_shape, dtype=np.float32) if hori_dist else None
    if rows is not None and dist_buffer is not None:
        dist_buffer.fill(np.nan)

    opts = hz_opts()
    opts.device = device
    opts.verbose = max(int(bool(verbose)), int(_verbose))      # _verbose = 2, 3: diagnostics of the library to stderr
    opts.top_nodes = _top_nodes
    opts.regroup = _regroup
    opts.no_hit_cache = 0 if _hit_cache else 1
    opts.chunk_rows = _chunk_rows
    # True: certificates when the scene allows them; False: never; "force": even for a mesh that is not a height field (tests)
    opts.no_near_skip = -1 if _near_skip == "force" else (0 if _near_skip else 1)
    opts.level_stack = int(_level_stack)      # True / 1: level stack from the start; -n: fast stack of n entries (tests)
    # schedule of the launches (results never depend on it; tests run the parity cases under several: schedule_overrides)
    opts.left_min = int(_left_min or schedule_overrides.get("left_min", 0))            # leftover cells: byte l = hand-over threshold of level l; 0: default; < 0: off
    opts.persist_grid = int(_persist_grid or schedule_overrides.get("persist_grid", 0))    # 0: persistent waves; < 0: one tile per workgroup; n > 0: n workgroups
    opts.left_cap_test = int(schedule_overrides.get("left_cap_test", 0))
    opts.left_tune = int(schedule_overrides.get("left_tune", 0))
    n_verify = int(_verify_near)              # False / 0: off; True / 1: every shortened ray; N: one of every N (rounded up to 2^k)
    if n_verify < 0 or n_verify != _verify_near:
        raise ValueError("_verify_near must be a non-negative integer (or a bool)")
    opts.verify_near = n_verify
    opts.skip_hori = 1 if (svf_only or topo_only) else 0
    opts.count_work = int(bool(count_work))
    if rows is not None:
        if len(rows) != 2 or not (0 <= int(rows[0]) < int(rows[1]) <= dim_in_0):
            raise ValueError("'rows' must be (begin, end) with 0 <= begin < end <= %d" % dim_in_0)
        opts.row_begin, opts.row_end = int(rows[0]), int(rows[1])
    svf = None
    if svf_vec_tilt is not None:
        _check_f32(svf_vec_tilt, 3, "svf_vec_tilt")
        if azim_num < 2:      # the azimuth spacing azim[1] - azim[0] does not exist (topo_param.pyx:433)
            raise ValueError("sky view factor needs azim_num >= 2")
        if svf_vec_tilt.shape != vec_norm.shape:
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
        svf_vec_tilt = np.ascontiguousarray(svf_vec_tilt)
        svf = np.full((dim_in_0, dim_in_1), np.nan, dtype=np.float32)
        opts.svf = ptr(svf)
        opts.vec_tilt = ptr(svf_vec_tilt)
    maps, topo_out = None, None
    if names is not None:
        # NaN outside a row slab, as for the SVF; "svf" goes through hz_opts.svf, the others through hz_topo_out
        maps = {n: np.full((dim_in_0, dim_in_1), np.nan, dtype=np.float32) for n in TOPO_NAMES if n in names}
        if tilted:
            topo_vec_tilt = np.ascontiguousarray(topo_vec_tilt)
            opts.vec_tilt = ptr(topo_vec_tilt)
        if "svf" in maps:
            opts.svf = ptr(maps["svf"])
        if "vsf" in maps or "openness" in maps:
            topo_out = hz_topo_out(ptr(maps.get("vsf")), ptr(maps.get("openness")))
    stats = hz_stats()
    L = _lib.lib()

    def run(o, st):
        # (the _ex entry points only when hz_topo_out has a map: every other call reaches the library as before)
        ex = () if topo_out is None else (C.byref(topo_out),)
        if planes or q16:                         # (the planes and q16 forms always take the `topo` argument)
            ex = ex or (None,)
        lay = (int(planes),) if q16 else ()       # (the q16 forms: `int planes` after hori_q)
        if hori_dist:                             # (the _dist forms: `int hori_kind` and `dist_buffer` after hori)
            ex = ex or (None,)
            lay = (_hori_kind(planes, q16), ptr(dist_buffer))
        if scene is None:
            return (L.hz_horizon_gridded_dist if hori_dist else L.hz_horizon_gridded_q16 if q16 else L.hz_horizon_gridded_planes if planes
                    else L.hz_horizon_gridded_ex if ex else L.hz_horizon_gridded)(
                ptr(vert_grid), dem_dim_0, dem_dim_1, ptr(vec_norm), ptr(vec_north),
                offset_0, offset_1, ptr(hori_buffer), *lay, dim_in_0, dim_in_1, azim_num,
                dist_search, hori_acc, ray_algorithm.encode("utf-8"),
                geom_type.encode("utf-8"), ptr(vert_simp), num_vert_simp,
                ptr(tri_ind_simp), num_tri_simp, elev_ang_low_lim, ptr(mask),
                hori_fill, ray_org_elev, C.byref(o), *ex, C.byref(st))
        o.device = scene.device
        return (L.hz_horizon_gridded_scene_dist if hori_dist else L.hz_horizon_gridded_scene_q16 if q16 else L.hz_horizon_gridded_scene_planes if planes
                else L.hz_horizon_gridded_scene_ex if ex else L.hz_horizon_gridded_scene)(
            scene._h, ptr(vec_norm), ptr(vec_north), offset_0, offset_1,
            ptr(hori_buffer), *lay, dim_in_0, dim_in_1, azim_num, dist_search, hori_acc,
            ray_algorithm.encode("utf-8"), elev_ang_low_lim, ptr(mask), hori_fill,
            ray_org_elev, C.byref(o), *ex, C.byref(st))

    if devices is None:
        rc = run(opts, stats)
    else:
        # one host thread per GPU, one row slab each (ctypes releases the GIL during the call;
        # the library keeps its error string and build arenas per thread)
        import threading
        from .dist import row_slabs
        if scene is not None or rows is not None:
            raise ValueError("'devices' cannot be combined with 'scene' or 'rows'")
        devs = list(range(_lib.device_count())) if isinstance(devices, str) and devices == "all" \
            else [int(d) for d in devices]
        if not devs:
            raise ValueError("'devices' is empty")
        slabs = [sl for sl in row_slabs(mask, len(devs))]
        part, errs = [None] * len(devs), []

        def work(idx):
            b, e = slabs[idx]
            if e <= b:
                return
            o = hz_opts.from_buffer_copy(opts)
            o.device, o.row_begin, o.row_end = devs[idx], b, e
            st = hz_stats()
            try:
                _lib.check(run(o, st))
                part[idx] = st
            except Exception as exc:      # re-raised in the calling thread
                errs.append(exc)
        threads = [threading.Thread(target=work, args=(i,)) for i in range(len(devs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errs:
            raise errs[0]
        for st in part:                    # counts add up, times are the slowest device's
            if st is None:
                continue
            for name, _ in hz_stats._fields_:
                a, b = getattr(stats, name), getattr(st, name)
                setattr(stats, name, max(a, b) if name.startswith("t_") or name in ("bvh_height", "elev_num", "scene_bytes") else a + b)
        rc = 0
    _lib.check(rc)
    last_stats = stats.as_dict()

    # Recompute azimuth (horizon.pyx:191-195)
    azim = np.empty(azim_num, dtype=np.float32)
    for i in range(azim_num):
        azim[i] = ((2 * np.pi) / azim_num * i)

    head = (hori_buffer, dist_buffer, azim) if hori_dist else (hori_buffer, azim)
    if maps is not None:
        return head + (maps,)
    if svf is not None:
        return head + (svf,)
    return head


def horizon_distance(vert_grid, dem_dim_0, dem_dim_1, vec_norm, vec_north, offset_0, offset_1,
                     hori, dist_search, hori_acc=0.25, geom_type="grid",
                     vert_simp=np.array([0.0, 0.0, 0.0, 0.0], dtype=np.float32),
                     num_vert_simp=1,
                     tri_ind_simp=np.array([0, 0, 0, 0], dtype=np.int32),
                     num_tri_simp=1, elev_ang_low_lim=-15.0, mask=None, ray_org_elev=0.01,
                     *, device=0, scene=None, layout="cell_major", rows=None, _chunk_rows=0):
    """Distance to the horizon for a gridded horizon (not in the reference, which has it for locations only).

    ``hori`` is a horizon of the inner domain as ``horizon_gridded`` returns it: float32 [radian] or the uint16 codes of
    ``quantise``, (y, x, azim_num) or, with ``layout="azim_major"``, (azim_num, y, x); ``azim_num`` is read from its shape.
    The other arguments are those ``hori`` was computed with (``hori_acc``, ``elev_ang_low_lim`` and ``dist_search`` fix the
    elevation table and the ray length).  Returns the distance [metre], float32 of the shape of ``hori``.

    Meaning (clause 16), that of the reference's ``hori_dist_out``: the closest hit of the last ray
    that hit.  For a cell with ``mask == 1`` and a horizon value h (a code is decoded first), the ray is the one of the
    table entry ``hori_acc`` (five entries) below the last entry that is <= h -- for ``guess_constant`` exactly the last
    ray that hit -- and the distance is that of the closest triangle (DEM mesh or outer TIN) within ``dist_search``.  A
    nearer, lower ridge that also rises above h - ``hori_acc`` is what is reported, not the far range behind it.  NaN where
    that ray hits nothing (directions in which a small domain has no terrain), where h is NaN (outside a ``rows`` slab)
    and where ``mask != 1``.

    Keyword-only: ``device``, ``scene`` (a prebuilt ``Scene``), ``layout``, ``rows`` ((begin, end) slab of inner-domain rows to
    compute; the rest of the result is NaN)."""
    global last_stats
    _check_f32(vert_grid, 1, "vert_grid")
    _check_f32(vec_norm, 3, "vec_norm")
    _check_f32(vec_north, 3, "vec_north")
    _check_f32(vert_simp, 1, "vert_simp")
    if not isinstance(tri_ind_simp, np.ndarray) or tri_ind_simp.ndim != 1 or tri_ind_simp.dtype != np.int32:
        raise ValueError("Buffer dtype mismatch, expected 'int32_t' for tri_ind_simp")
    if mask is not None and (not isinstance(mask, np.ndarray) or mask.ndim != 2):
        raise ValueError("Buffer has wrong number of dimensions (expected 2) for mask")
    if not isinstance(hori, np.ndarray):
        raise TypeError("Argument 'hori' has incorrect type (expected numpy.ndarray, got %s)" % type(hori).__name__)
    if hori.ndim != 3:
        raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % hori.ndim)
    if hori.dtype not in (np.float32, np.uint16):
        raise ValueError("Buffer dtype mismatch, expected 'float32_t' or 'uint16_t' but got '%s'" % hori.dtype.name)
    planes = check_layout(layout)
    if mask is None:
        mask = np.ones(vec_norm.shape[:2], dtype=np.uint8)
    dim_in_0, dim_in_1 = vec_norm.shape[0], vec_norm.shape[1]
    azim_num = hori.shape[0] if planes else hori.shape[2]
    V.run((
        (ValueError, "inconsistency between input arguments vert_grid, dem_dim_0 and dem_dim_1",
         lambda: not V.fits_grid(len(vert_grid), dem_dim_0, dem_dim_1)),
        (ValueError, "inconsistency between input arguments dem_dim_0, dem_dim_1, offset_0, offset_1 and vec_norm",
         lambda: not V.window_inside(offset_0, offset_1, vec_norm.shape, dem_dim_0, dem_dim_1)),
        (ValueError, V.MSG_NORTH, lambda: not V.same_leading_shape((vec_norm, vec_north), 3, 3)),
        (ValueError, "Inconsistent/incorrect shape of 'hori'",
         lambda: azim_num < 1 or (hori.shape[1:] if planes else hori.shape[:2]) != (dim_in_0, dim_in_1)),
        (ValueError, V.MSG_GEOM, lambda: geom_type not in V.GEOMETRIES),
        (ValueError, "inconsistency between input arguments vert_simp and num_vert_simp", lambda: len(vert_simp) < num_vert_simp * 3),
        (ValueError, "inconsistency between input arguments tri_ind_simp and num_tri_simp", lambda: len(tri_ind_simp) < num_tri_simp * 3),
        (ValueError, "triangle indices of simplified outer domain exceed number of vertices",
         lambda: tri_ind_simp.max() > num_vert_simp - 1),
        (ValueError, V.MSG_ACC, lambda: hori_acc > 10.0),
        (ValueError, "shape of mask is inconsistent with other input", lambda: mask.shape[:2] != vec_norm.shape[:2]),
        (TypeError, V.MSG_MASK_TYPE, lambda: mask.dtype != "uint8"),
        (TypeError, V.MSG_ELEV, lambda: ray_org_elev < 0.005),
        (ValueError, V.MSG_DIM_LIMIT, lambda: max(dem_dim_0, dem_dim_1) > V.DIM_LIMIT),
    ))
    opts = hz_opts()
    opts.device = device if scene is None else scene.device
    opts.chunk_rows = _chunk_rows
    if rows is not None:
        if len(rows) != 2 or not (0 <= int(rows[0]) < int(rows[1]) <= dim_in_0):
            raise ValueError("'rows' must be (begin, end) with 0 <= begin < end <= %d" % dim_in_0)
        opts.row_begin, opts.row_end = int(rows[0]), int(rows[1])

    vert_grid = np.ascontiguousarray(vert_grid)
    vec_norm = np.ascontiguousarray(vec_norm)
    vec_north = np.ascontiguousarray(vec_north)
    vert_simp = np.ascontiguousarray(vert_simp)
    tri_ind_simp = np.ascontiguousarray(tri_ind_simp)
    mask = np.ascontiguousarray(mask)
    hori = np.ascontiguousarray(hori)
    dist = np.empty(hori.shape, dtype=np.float32)
    if rows is not None:
        dist.fill(np.nan)           # only a slab is written
    kind = _hori_kind(planes, hori.dtype == np.uint16)
    stats = hz_stats()
    L = _lib.lib()
    if scene is None:
        rc = L.hz_horizon_distance(
            ptr(vert_grid), dem_dim_0, dem_dim_1, ptr(hori), kind, ptr(dist), ptr(vec_norm), ptr(vec_north),
            offset_0, offset_1, dim_in_0, dim_in_1, azim_num, dist_search, hori_acc, geom_type.encode("utf-8"),
            ptr(vert_simp), num_vert_simp, ptr(tri_ind_simp), num_tri_simp, elev_ang_low_lim, ptr(mask), ray_org_elev,
            C.byref(opts), C.byref(stats))
    else:
        rc = L.hz_horizon_distance_scene(
            scene._h, ptr(hori), kind, ptr(dist), ptr(vec_norm), ptr(vec_north), offset_0, offset_1,
            dim_in_0, dim_in_1, azim_num, dist_search, hori_acc, elev_ang_low_lim, ptr(mask), ray_org_elev,
            C.byref(opts), C.byref(stats))
    _lib.check(rc)
    last_stats = stats.as_dict()
    return dist


def horizon_locations(vert_grid, dem_dim_0, dem_dim_1, coords, vec_norm, vec_north,
                      dist_search, azim_num=360, hori_acc=0.25,
                      ray_algorithm="binary_search", geom_type="grid",
                      elev_ang_low_lim=-89.98,
                      ray_org_elev=np.array([0.01], dtype=np.float32),
                      hori_dist_out=False, *, device=0, verbose=False, scene=None):
    """Horizon computation for arbitrary locations.

    Parameters, units and return values are those of the reference
    (horizon.pyx:233-276): returns ``hori_buffer`` float32 (number of locations,
    azim_num) [radian] and ``azim``; with ``hori_dist_out`` also the distance to the
    horizon [metre] as second value.  Keyword-only extras: ``device``, ``verbose``, ``scene``."""
    global last_stats
    _check_f32(vert_grid, 1, "vert_grid")
    _check_f32(coords, 2, "coords")
    _check_f32(vec_norm, 2, "vec_norm")
    _check_f32(vec_north, 2, "vec_north")
    _check_f32(ray_org_elev, 1, "ray_org_elev")

    # Consistency and validity of the arguments: the reference's checks, classes, messages and order (horizon.pyx:279-312)
    V.run((
        (ValueError, "inconsistency between input arguments vert_grid, dem_dim_0 and dem_dim_1",
         lambda: not V.fits_grid(len(vert_grid), dem_dim_0, dem_dim_1)),
        (ValueError, "'number of dimensions and/or dimension length(s) of 'coords' incorrect",
         lambda: coords.ndim != 2 or coords.shape != (vec_norm.shape[0], 3)),
        (ValueError, V.MSG_NORTH, lambda: not V.same_leading_shape((vec_norm, vec_north), 2, 2)),
        (ValueError, V.MSG_ALG, lambda: ray_algorithm not in V.ALGORITHMS),
        (ValueError, V.MSG_GEOM, lambda: geom_type not in V.GEOMETRIES),
        (ValueError, V.MSG_ACC, lambda: hori_acc > 10.0),
        (ValueError, "length of array 'ray_org_elev' must be either one or correspond to the number of locations",
         lambda: len(ray_org_elev) not in (1, coords.shape[0])),
        (TypeError, V.MSG_ELEV, lambda: ray_org_elev.min() < 0.005),
        (TypeError, "horizon detection algorithm 'guess_constant' not implemented for horizon distance computation",
         lambda: bool(hori_dist_out) and ray_algorithm == "guess_constant"),
        (ValueError, V.MSG_DIM_LIMIT, lambda: max(dem_dim_0, dem_dim_1) > V.DIM_LIMIT),
    ))

    # Repeat array 'ray_org_elev' if necessary (horizon.pyx:315-316)
    if len(ray_org_elev) != coords.shape[0]:
        ray_org_elev = np.repeat(ray_org_elev, coords.shape[0])

    vert_grid = np.ascontiguousarray(vert_grid)
    coords = np.ascontiguousarray(coords)
    vec_norm = np.ascontiguousarray(vec_norm)
    vec_north = np.ascontiguousarray(vec_north)
    ray_org_elev = np.ascontiguousarray(ray_org_elev)

    num_loc = vec_norm.shape[0]
    hori_buffer = np.empty((num_loc, azim_num), dtype=np.float32)
    hori_buffer.fill(np.nan)
    hori_dist_buffer = np.empty((num_loc if hori_dist_out else 1, azim_num), dtype=np.float32)
    hori_dist_buffer.fill(np.nan)

    opts = hz_opts()
    opts.device = device if scene is None else scene.device
    opts.verbose = int(bool(verbose))
    stats = hz_stats()
    L = _lib.lib()
    if num_loc == 0:    # the reference's loop over locations simply does not run
        rc = 0
    elif scene is None:
        rc = L.hz_horizon_locations(
            ptr(vert_grid), dem_dim_0, dem_dim_1, ptr(coords), ptr(vec_norm), ptr(vec_north),
            ptr(hori_buffer), ptr(hori_dist_buffer) if hori_dist_out else None, num_loc, azim_num,
            dist_search, hori_acc, ray_algorithm.encode("utf-8"), geom_type.encode("utf-8"),
            elev_ang_low_lim, ptr(ray_org_elev), int(bool(hori_dist_out)), C.byref(opts), C.byref(stats))
    else:
        rc = L.hz_horizon_locations_scene(
            scene._h, ptr(coords), ptr(vec_norm), ptr(vec_north), ptr(hori_buffer),
            ptr(hori_dist_buffer) if hori_dist_out else None, num_loc, azim_num, dist_search, hori_acc,
            ray_algorithm.encode("utf-8"), elev_ang_low_lim, ptr(ray_org_elev), int(bool(hori_dist_out)),
            C.byref(opts), C.byref(stats))
    _lib.check(rc)
    last_stats = stats.as_dict()

    azim = np.empty(azim_num, dtype=np.float32)
    for i in range(azim_num):
        azim[i] = ((2 * np.pi) / azim_num * i)

    if hori_dist_out:
        return hori_buffer, hori_dist_buffer, azim
    else:
        return hori_buffer, azim


def horizon_tables(azim_num, hori_acc, elev_ang_low_lim):
    """The trig tables the library builds on the host (for bit-for-bit checks)."""
    L = _lib.lib()
    n = C.c_int(0)
    _lib.check(L.hz_horizon_tables(azim_num, hori_acc, elev_ang_low_lim, None, None, 0,
                                   None, None, None, C.byref(n)))
    out = {k: np.empty(azim_num, np.float32) for k in ("azim_sin", "azim_cos")}
    out.update({k: np.empty(n.value, np.float32) for k in ("elev_ang", "elev_sin", "elev_cos")})
    _lib.check(L.hz_horizon_tables(azim_num, hori_acc, elev_ang_low_lim, ptr(out["azim_sin"]),
                                   ptr(out["azim_cos"]), n.value, ptr(out["elev_ang"]),
                                   ptr(out["elev_sin"]), ptr(out["elev_cos"]), C.byref(n)))
    out["elev_num"] = n.value
    return out
