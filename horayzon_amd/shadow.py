"""horayzon.shadow -- shadow mask and direct-shortwave correction on MI355X.

Host-side mirror of the reference's ``cdef class Terrain``
(horayzon/shadow.pyx:17-200): same method names, argument order, defaults,
validation and exception classes; the scene (LBVH) and all per-cell inputs
live in HBM for the lifetime of the object (the reference keeps raw host
pointers, shadow_comp.cpp:332-346).
"""
import ctypes as C

import numpy as np

from . import _lib
from . import _validate as V
from ._lib import hz_stats, ptr
from ._validate import contiguous as _contiguous


def _typed(a, dtype, ndim, name):
    if not isinstance(a, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)"
                        % (name, type(a).__name__))
    if a.ndim != ndim:
        raise ValueError("Buffer has wrong number of dimensions (expected %d, got %d)" % (ndim, a.ndim))
    if a.dtype != dtype:
        raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s'"
                         % (np.dtype(dtype).name, a.dtype.name))


def _accumulate_types(obj, sun_positions, weights, outs):
    """The argument types of ``accumulate``, in the order they are checked."""
    obj._array_arg(sun_positions, 2, "sun_positions")
    if weights is not None:
        obj._array_arg(weights, 1, "weights")
    for name, buf in outs:
        if buf is not None:
            obj._array_arg(buf, 2, name)


def _accumulate_checks(sun_positions, weights, outs):
    """The check list both ``accumulate`` methods share (``V.run``; HorizonTerrain appends its map checks)."""
    given = [buf for _, buf in outs if buf is not None]
    arrays = [sun_positions] + ([weights] if weights is not None else []) + given
    return (
        (ValueError, "at least one of 'sw_dir_cor_sum' and 'sunlit_sum' must be given", lambda: not given),
        (ValueError, "array 'sun_positions' has incorrect shape",
         lambda: sun_positions.shape[1] != 3 or sun_positions.shape[0] < 1),
        (ValueError, "array 'weights' has incorrect shape",
         lambda: weights is not None and weights.shape[0] != sun_positions.shape[0]),
        (ValueError, "not all input arrays are C-contiguous", lambda: not all(_contiguous(a) for a in arrays)),
        (ValueError, "'sw_dir_cor_sum' and 'sunlit_sum' must be different arrays",
         lambda: len(given) == 2 and ptr(given[0]) == ptr(given[1])),
    )


def _sw_dir_cor_coarse(obj, entry, sun_positions, pixel_per_gc, f_cor, sunlit_frac):
    """``sw_dir_cor_coarse`` of both classes: the checks, then the entry point ``entry`` of the library."""
    outs = (("f_cor", f_cor), ("sunlit_frac", sunlit_frac))
    obj._array_arg(sun_positions, 2, "sun_positions")
    p0, p1 = obj._pixel_per_gc(pixel_per_gc)
    for name, buf in outs:
        if buf is not None:
            obj._array_arg(buf, 3, name)
    if obj._shape is None:
        raise _lib.HorayzonHipError("%s is not initialised" % obj._NAME)
    given = [buf for _, buf in outs if buf is not None]
    dim_0, dim_1 = obj._shape

    def coarse_shape():
        return (sun_positions.shape[0], dim_0 // p0, dim_1 // p1)
    V.run((
        (ValueError, "at least one of 'f_cor' and 'sunlit_frac' must be given", lambda: not given),
        (ValueError, "array 'sun_positions' has incorrect shape",
         lambda: sun_positions.shape[1] != 3 or sun_positions.shape[0] < 1),
        (ValueError, "'pixel_per_gc' (%d, %d) must be positive and divide the inner domain (%d, %d)" % (p0, p1, dim_0, dim_1),
         lambda: p0 < 1 or p1 < 1 or p0 > dim_0 or p1 > dim_1 or dim_0 % p0 != 0 or dim_1 % p1 != 0),
        (ValueError, "array 'f_cor' has incorrect shape",
         lambda: f_cor is not None and tuple(f_cor.shape) != coarse_shape()),
        (ValueError, "array 'sunlit_frac' has incorrect shape",
         lambda: sunlit_frac is not None and tuple(sunlit_frac.shape) != coarse_shape()),
        (ValueError, "not all input arrays are C-contiguous", lambda: not all(_contiguous(a) for a in [sun_positions] + given)),
        (ValueError, "'f_cor' and 'sunlit_frac' must be different arrays",
         lambda: len(given) == 2 and ptr(given[0]) == ptr(given[1])),
    ))
    st = hz_stats()
    _lib.check(getattr(_lib.lib(), entry)(
        obj._h, ptr(sun_positions), sun_positions.shape[0], p0, p1, ptr(f_cor), ptr(sunlit_frac), C.byref(st)))
    obj.last_stats = st.as_dict()


class Terrain:
    _NAME = "Terrain"                   # in messages

    def __init__(self, *, device=0):
        self._h = C.c_void_p()
        self._shape = None
        self.device = device
        self.last_stats = None
        _lib.check(_lib.lib().hz_terrain_create(device, C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().hz_terrain_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def initialise(self, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                   vec_tilt, vec_norm, surf_enl_fac, elevation, mask,
                   geom_type="grid", sw_dir_cor_fill=np.nan, ang_max=89.0,
                   refrac_cor=False, *, scene=None):
        """Initialise Terrain class with Digital Elevation Model (DEM) data.

        Arguments as in the reference (shadow.pyx:40-85).  ``scene`` (keyword
        only, not in the reference) reuses a prebuilt ``Scene``."""
        _typed(vert_grid, np.float32, 1, "vert_grid")
        _typed(vec_tilt, np.float32, 3, "vec_tilt")
        _typed(vec_norm, np.float32, 3, "vec_norm")
        _typed(surf_enl_fac, np.float32, 2, "surf_enl_fac")
        _typed(elevation, np.float32, 2, "elevation")
        _typed(mask, np.uint8, 2, "mask")

        # Consistency and validity of the arguments: the reference's checks, classes, messages and order (shadow.pyx:87-133)
        cell_arrays = (vec_tilt[..., 0], surf_enl_fac, elevation, mask) if vec_tilt.ndim == 3 else (surf_enl_fac, elevation, mask)
        V.run((
            (ValueError, "inconsistency between input arguments 'vert_grid', 'dem_dim_0' and 'dem_dim_1'",
             lambda: not V.fits_grid(len(vert_grid), dem_dim_0, dem_dim_1)),
            (ValueError, "inconsistency between input arguments 'dem_dim_0', 'dem_dim_1', 'offset_0', 'offset_1' and 'vec_norm'",
             lambda: not V.window_inside(offset_0, offset_1, vec_tilt.shape, dem_dim_0, dem_dim_1)),
            (ValueError, "Inconsistent/incorrect shape of 'vec_tilt' and/or 'vec_norm'",
             lambda: not V.same_leading_shape((vec_tilt, vec_norm), 3, 3) or vec_tilt.shape[2] != 3),
            (ValueError, "Inconsistent/incorrect shape of 'surf_enl_fac',  'elevation' and/or 'mask'",
             lambda: not V.same_leading_shape(cell_arrays, 2, 2)),
            (ValueError, "not all input arrays are C-contiguous",
             lambda: not all(a.flags["C_CONTIGUOUS"] for a in (vert_grid, vec_tilt, vec_norm, surf_enl_fac, elevation, mask))),
            (ValueError, "Vectors in 'vec_tilt' and/or 'vec_norm' are not normalised",
             lambda: not (V.unit_vectors(vec_tilt) and V.unit_vectors(vec_norm))),
            (ValueError, V.MSG_GEOM, lambda: geom_type not in V.GEOMETRIES),
            (TypeError, V.MSG_MASK_TYPE, lambda: mask.dtype != "uint8"),
            (TypeError, "'ang_max' must be in the range [85.0, 89.99]", lambda: ang_max < 85.0 or ang_max > 89.99),
            (ValueError, V.MSG_DIM_LIMIT, lambda: max(dem_dim_0, dem_dim_1) > V.DIM_LIMIT),
        ))

        L = _lib.lib()
        st = hz_stats()
        if scene is None:
            rc = L.hz_terrain_initialise(
                self._h, ptr(vert_grid), dem_dim_0, dem_dim_1, offset_0, offset_1,
                ptr(vec_tilt), ptr(vec_norm), vec_tilt.shape[0], vec_tilt.shape[1],
                ptr(surf_enl_fac), ptr(elevation), ptr(mask), geom_type.encode("utf-8"),
                sw_dir_cor_fill, ang_max, int(refrac_cor), C.byref(st))
        else:
            self._scene = scene   # keep the borrowed scene alive
            self.device = scene.device   # the terrain follows the scene's GPU (hz_terrain_initialise_scene)
            rc = L.hz_terrain_initialise_scene(
                self._h, scene._h, offset_0, offset_1, ptr(vec_tilt), ptr(vec_norm),
                vec_tilt.shape[0], vec_tilt.shape[1], ptr(surf_enl_fac), ptr(elevation),
                ptr(mask), sw_dir_cor_fill, ang_max, int(refrac_cor))
        _lib.check(rc)
        self._shape = (vec_tilt.shape[0], vec_tilt.shape[1])
        self.last_stats = st.as_dict()

    def _require_initialised(self):
        if self._shape is None:
            raise _lib.HorayzonHipError("%s is not initialised" % self._NAME)

    def _call(self, symbol, *args):
        """The library's entry point `symbol` on the handle; the hz_stats it fills in become ``last_stats``."""
        st = hz_stats()
        _lib.check(getattr(_lib.lib(), symbol)(self._h, *args, C.byref(st)))
        self.last_stats = st.as_dict()

    def _check_out(self, buf, name):
        self._require_initialised()
        if tuple(buf.shape[-2:]) != self._shape:
            raise ValueError("array '%s' has incorrect shape" % name)

    def shadow(self, sun_position, shadow_buffer):
        """Compute shadow mask for specified sun position
        (0: illuminated, 1: self-shaded, 2: terrain-shaded, 3: masked)."""
        _typed(sun_position, np.float32, 1, "sun_position")
        _typed(shadow_buffer, np.uint8, 2, "shadow_buffer")
        # Check consistency and validity of input arguments (shadow.pyx:165-168)
        if (sun_position.ndim != 1) or (sun_position.size != 3):
            raise ValueError("array 'sun_position' has incorrect shape")
        if not shadow_buffer.flags["C_CONTIGUOUS"]:
            raise ValueError("array 'shadow_buffer' is not C-contiguous")
        self._check_out(shadow_buffer, "shadow_buffer")
        self._call("hz_terrain_shadow", ptr(np.ascontiguousarray(sun_position)), ptr(shadow_buffer))

    def sw_dir_cor(self, sun_position, sw_dir_cor_buffer):
        """Compute shortwave correction factor for specified sun position."""
        _typed(sun_position, np.float32, 1, "sun_position")
        _typed(sw_dir_cor_buffer, np.float32, 2, "sw_dir_cor_buffer")
        # Check consistency and validity of input arguments (shadow.pyx:195-198)
        if (sun_position.ndim != 1) or (sun_position.size != 3):
            raise ValueError("array 'sun_position' has incorrect shape")
        if not sw_dir_cor_buffer.flags["C_CONTIGUOUS"]:
            raise ValueError("array 'sw_dir_cor_buffer' is not C-contiguous")
        self._check_out(sw_dir_cor_buffer, "sw_dir_cor_buffer")
        self._call("hz_terrain_sw_dir_cor", ptr(np.ascontiguousarray(sun_position)), ptr(sw_dir_cor_buffer))

    def count_work(self, on=True):
        """Additive: later calls also count BVH node visits / triangle tests (``last_stats``; slower)."""
        _lib.check(_lib.lib().hz_terrain_count_work(self._h, int(bool(on))))

    # --- additive batch API (not in the reference): many sun positions, one call ------
    @staticmethod
    def _batch_out(buf, np_dtype, name):
        """The batch forms (additive API) also take torch tensors in HBM: outputs of 144 sun positions of a
        3601^2 tile are 1.8 GB / 7.3 GB and usually consumed on the GPU."""
        if isinstance(buf, np.ndarray):
            _typed(buf, np_dtype, 3, name)
            if not buf.flags["C_CONTIGUOUS"]:
                raise ValueError("array '%s' is not C-contiguous" % name)
            return
        if not hasattr(buf, "data_ptr"):
            raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray or torch.Tensor, got %s)"
                            % (name, type(buf).__name__))
        if buf.dim() != 3:
            raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % buf.dim())
        if str(buf.dtype).split(".")[-1] != np.dtype(np_dtype).name:
            raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s'" % (np.dtype(np_dtype).name, buf.dtype))
        if not buf.is_contiguous():
            raise ValueError("array '%s' is not C-contiguous" % name)

    def shadow_batch(self, sun_positions, shadow_buffers):
        """``shadow`` for sun_positions f32[num][3] -> shadow_buffers u8[num][y][x] (NumPy or torch/HBM)."""
        _typed(sun_positions, np.float32, 2, "sun_positions")
        self._batch_out(shadow_buffers, np.uint8, "shadow_buffers")
        if sun_positions.shape[1] != 3 or shadow_buffers.shape[0] != sun_positions.shape[0]:
            raise ValueError("array 'sun_positions' has incorrect shape")
        self._check_out(shadow_buffers, "shadow_buffers")
        self._call("hz_terrain_shadow_batch", ptr(np.ascontiguousarray(sun_positions)), sun_positions.shape[0],
                   ptr(shadow_buffers))

    def sw_dir_cor_batch(self, sun_positions, sw_dir_cor_buffers):
        """``sw_dir_cor`` for sun_positions f32[num][3] -> sw_dir_cor_buffers f32[num][y][x] (NumPy or torch/HBM)."""
        _typed(sun_positions, np.float32, 2, "sun_positions")
        self._batch_out(sw_dir_cor_buffers, np.float32, "sw_dir_cor_buffers")
        if sun_positions.shape[1] != 3 or sw_dir_cor_buffers.shape[0] != sun_positions.shape[0]:
            raise ValueError("array 'sun_positions' has incorrect shape")
        self._check_out(sw_dir_cor_buffers, "sw_dir_cor_buffers")
        self._call("hz_terrain_sw_dir_cor_batch", ptr(np.ascontiguousarray(sun_positions)), sun_positions.shape[0],
                   ptr(sw_dir_cor_buffers))

    # --- additive: weighted sums over many sun positions, no map per position -------------------------------------
    def _array_arg(self, buf, ndim, name, np_dtype=np.float32, owner="Terrain"):
        """Array argument of the additive calls: a NumPy array, or a torch tensor on the object's GPU."""
        if isinstance(buf, np.ndarray):
            _typed(buf, np_dtype, ndim, name)
            return
        if not hasattr(buf, "data_ptr"):
            raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray or torch.Tensor, got %s)"
                            % (name, type(buf).__name__))
        if buf.dim() != ndim:
            raise ValueError("Buffer has wrong number of dimensions (expected %d, got %d)" % (ndim, buf.dim()))
        if str(buf.dtype).split(".")[-1] != np.dtype(np_dtype).name:
            raise ValueError("Buffer dtype mismatch, expected '%s' but got '%s'" % (np.dtype(np_dtype).name, buf.dtype))
        if buf.device.type != "cuda" or buf.device.index != self.device:
            raise ValueError("tensor '%s' is not on the %s's device (cuda:%d)" % (name, owner, self.device))

    def _given_outputs(self, outs):
        """The outputs that were given, out of the table ((name, buf, ndim, dtype), ...), after their types are checked."""
        for name, buf, ndim, dtype in outs:
            if buf is not None:
                self._array_arg(buf, ndim, name, dtype)
        return [buf for _, buf, _, _ in outs if buf is not None]

    def accumulate(self, sun_positions, weights=None, *, sw_dir_cor_sum=None, sunlit_sum=None):
        """Weighted sums over sun_positions f32[S][3] (S >= 1) without a map per position:
        ``sw_dir_cor_sum`` = sum of weights[s] * sw_dir_cor(sun_positions[s]) and ``sunlit_sum`` = sum of weights[s] over
        the positions for which shadow() gives 0, per cell, accumulated in float64 in ascending s and rounded to float32
        once; masked cells get ``sw_dir_cor_fill``.  weights f32[S] (None: ones).  Outputs f32[y][x], NumPy or torch
        tensors on the Terrain's GPU; at least one.  Device memory besides the buffers does not grow with S
        (``last_stats["scratch_bytes"]``)."""
        outs = (("sw_dir_cor_sum", sw_dir_cor_sum), ("sunlit_sum", sunlit_sum))
        _accumulate_types(self, sun_positions, weights, outs)
        V.run(_accumulate_checks(sun_positions, weights, outs))
        for name, buf in outs:
            if buf is not None:
                self._check_out(buf, name)
        self._call("hz_terrain_accumulate", ptr(sun_positions), ptr(weights), sun_positions.shape[0],
                   ptr(sw_dir_cor_sum), ptr(sunlit_sum))

    # --- additive: block means per sun position (sub-grid look-up tables), no map per position ---------------------
    @staticmethod
    def _pixel_per_gc(pixel_per_gc):
        """(P0, P1) of an int or a pair of ints; anything else (bool included) is a TypeError."""
        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        if is_int(pixel_per_gc):
            return int(pixel_per_gc), int(pixel_per_gc)
        if isinstance(pixel_per_gc, (tuple, list)) and len(pixel_per_gc) == 2 and all(is_int(v) for v in pixel_per_gc):
            return int(pixel_per_gc[0]), int(pixel_per_gc[1])
        raise TypeError("Argument 'pixel_per_gc' has incorrect type (expected an int or a pair of ints, got %r)"
                        % (pixel_per_gc,))

    def sw_dir_cor_coarse(self, sun_positions, pixel_per_gc, *, f_cor=None, sunlit_frac=None):
        """Per sun position of sun_positions f32[S][3] (S >= 1), means over blocks of P0 x P1 cells of the inner domain
        (``pixel_per_gc``: an int P or a pair (P0, P1) that divide its shape), without a map per position:
        ``f_cor[s][I][J]`` = the mean of sw_dir_cor(sun_positions[s]) and ``sunlit_frac[s][I][J]`` = the fraction of cells
        for which shadow() gives 0, both over the unmasked cells of the block.  The sum is a float64 accumulator over the
        block's unmasked cells in row-major order, divided by their number in float64 and rounded to float32 once; a block
        without an unmasked cell gets ``sw_dir_cor_fill``.  Outputs f32[S][gy][gx], NumPy or torch tensors on the Terrain's
        GPU; at least one.  Device memory besides the outputs does not grow with S (``last_stats["scratch_bytes"]``)."""
        _sw_dir_cor_coarse(self, "hz_terrain_sw_dir_cor_coarse", sun_positions, pixel_per_gc, f_cor, sunlit_frac)


    # --- additive: line-of-sight maps from observer points ------------------------------------------------------------
    def viewshed(self, observers, *, visible=None, seen_count=None, cells_seen=None,
                 target_elev=0.05, max_dist=None, facing=True):
        """Which cells have a free line of sight to each point of observers f32[S][3] (S >= 1; the scene's ENU frame, the
        frame of ``sun_position``; NumPy or a torch tensor on the Terrain's GPU; finite): a mast, a camera, a candidate
        site.  Unlike a sun position the observer ends the ray, so terrain behind it blocks nothing.  Per observer and
        cell one code (clause 18) -- 0: in sight, 1: the tilted surface faces away (``facing``; no ray),
        2: terrain in between, 3: masked, 4: farther than ``max_dist`` (no ray) -- for the point ``target_elev`` [m]
        (>= 0.005) above the surface along ``vec_norm``; ``max_dist`` [m] is None or > 0; with ``facing=False`` back-facing
        cells are traced too.  Refraction is never applied.  Outputs, any subset, at least one: ``visible`` u8[S][y][x] the
        codes, ``seen_count`` i32[y][x] the number of observers that see the cell (masked cells: -1), ``cells_seen``
        i64[S] the number of cells each observer sees; NumPy or torch tensors on the Terrain's GPU.
        ``last_stats["num_rays"]`` is the number of rays traced.  ``last_stats["scratch_bytes"]``, the device memory the call
        allocates besides the buffers, does not grow with S; NumPy observers also go through the Terrain's own staging
        buffer (12 bytes per observer, at most 32768 observers at a time, kept with the object and not counted there).  The
        finiteness check of observers given as a tensor is a reduction on the GPU whose result is read back: one device
        synchronisation per call before the launches."""
        outs = (("visible", visible, 3, np.uint8), ("seen_count", seen_count, 2, np.int32),
                ("cells_seen", cells_seen, 1, np.int64))
        self._array_arg(observers, 2, "observers")
        given = self._given_outputs(outs)
        if not V.is_number(target_elev):
            raise TypeError("Argument 'target_elev' has incorrect type (expected a number, got %s)" % type(target_elev).__name__)
        if max_dist is not None and not V.is_number(max_dist):
            raise TypeError("Argument 'max_dist' has incorrect type (expected a number or None, got %s)" % type(max_dist).__name__)
        if not isinstance(facing, (bool, np.bool_)):
            raise TypeError("Argument 'facing' has incorrect type (expected bool, got %s)" % type(facing).__name__)
        V.run((
            V.some_output_given(outs, given),
            (ValueError, "array 'observers' has incorrect shape", lambda: observers.shape[1] != 3 or observers.shape[0] < 1),
            (ValueError, "array 'visible' has incorrect shape",
             lambda: visible is not None and visible.shape[0] != observers.shape[0]),
            (ValueError, "array 'cells_seen' has incorrect shape",
             lambda: cells_seen is not None and cells_seen.shape[0] != observers.shape[0]),
            V.all_contiguous(lambda: [observers] + given),
            V.distinct_outputs(outs, given),
            (ValueError, "'target_elev' must be at least 0.005 m", lambda: not (np.isfinite(target_elev) and target_elev >= 0.005)),
            (ValueError, "'max_dist' must be None or greater than 0", lambda: max_dist is not None and not np.float32(max_dist) > 0),
            (ValueError, "array 'observers' has non-finite entries", lambda: not V.all_finite(observers)),
        ))
        for name, buf in (("visible", visible), ("seen_count", seen_count)):
            if buf is not None:
                self._check_out(buf, name)
        self._require_initialised()
        self._call("hz_terrain_viewshed", ptr(observers), observers.shape[0], float(target_elev),
                   0.0 if max_dist is None else float(max_dist), int(bool(facing)), ptr(visible), ptr(seen_count), ptr(cells_seen))

    # --- additive: depth images of the terrain from observer points -----------------------------------------------------
    def panorama(self, observers, azim, elev, max_dist, *, dist=None, point=None, hits=None,
                 vec_north=None, vec_norm=None):
        """Looking out from each point of observers f32[S][3] (as in ``viewshed``: the scene's frame; NumPy or a torch
        tensor on the Terrain's GPU; finite) in the directions azim f32[A] x elev f32[E] (NumPy, radians, finite, A >= 1,
        E >= 1, E * A <= 2**30; azimuth clockwise from north, elevation in [-pi/2, pi/2] as float32; any order or spacing):
        how far away is the terrain, and where does the ray land?  One closest-hit ray of length ``max_dist`` [m] (a
        number, finite and > 0 as float32) per observer and pixel, against the whole scene (clause
        20); ``mask``, ``vec_tilt`` and the inner-domain offsets play no part and refraction is never applied.
        ``vec_north`` / ``vec_norm`` f32[S][3] (NumPy, unit vectors, both or neither) give each observer's local frame, e.g.
        on a curved DEM; with neither, north = (0, 1, 0) and norm = (0, 0, 1).  Outputs, any subset, at least one, every
        element written: ``dist`` f32[S][E][A] the distance to the closest triangle, NaN where nothing is hit within
        ``max_dist``; ``point`` f32[S][E][A][3] the hit point observer + direction * distance (NaN x 3 where nothing is
        hit); ``hits`` i64[S] the pixels with a hit; NumPy or torch tensors on the Terrain's GPU.  An observer on the
        surface hits it at distance 0.0.  ``last_stats["num_rays"]`` is S * E * A.  Observers go in chunks: NumPy images
        are staged on the device one chunk at a time (at most 256 MiB, or one observer's images), so
        ``last_stats["scratch_bytes"]`` does not grow with S.  The finiteness check of observers given as a tensor reads a
        reduction back from the GPU: one device synchronisation per call before the launches."""
        outs = (("dist", dist, 3, np.float32), ("point", point, 4, np.float32), ("hits", hits, 1, np.int64))
        self._array_arg(observers, 2, "observers")
        for name, tab in (("azim", azim), ("elev", elev)):
            _typed(tab, np.float32, 1, name)
        if not V.is_number(max_dist):
            raise TypeError("Argument 'max_dist' has incorrect type (expected a number, got %s)" % type(max_dist).__name__)
        given = self._given_outputs(outs)
        frames = [(name, v) for name, v in (("vec_north", vec_north), ("vec_norm", vec_norm)) if v is not None]
        for name, v in frames:
            _typed(v, np.float32, 2, name)

        def image_shape():
            return (observers.shape[0], elev.shape[0], azim.shape[0])
        half_pi = np.float32(np.pi / 2)
        with np.errstate(over="ignore"):
            tfar = np.float32(max_dist)                      # the ray length the kernel sees
        V.run((
            V.some_output_given(outs, given),
            (ValueError, "array 'observers' has incorrect shape", lambda: observers.shape[1] != 3 or observers.shape[0] < 1),
            (ValueError, "array 'azim' must have at least one entry", lambda: azim.shape[0] < 1),
            (ValueError, "array 'elev' must have at least one entry", lambda: elev.shape[0] < 1),
            (ValueError, "an image of 'elev' x 'azim' must not have more than 2**30 pixels",
             lambda: elev.shape[0] * azim.shape[0] > 2 ** 30),
            (ValueError, "array 'dist' has incorrect shape", lambda: dist is not None and tuple(dist.shape) != image_shape()),
            (ValueError, "array 'point' has incorrect shape",
             lambda: point is not None and tuple(point.shape) != image_shape() + (3,)),
            (ValueError, "array 'hits' has incorrect shape", lambda: hits is not None and hits.shape[0] != observers.shape[0]),
            (ValueError, "'vec_north' and 'vec_norm' must be given together", lambda: len(frames) == 1),
            (ValueError, "Inconsistent/incorrect shape of 'vec_north' and/or 'vec_norm'",
             lambda: any(tuple(v.shape) != (observers.shape[0], 3) for _, v in frames)),
            V.all_contiguous(lambda: [observers, azim, elev] + [v for _, v in frames] + given),
            V.distinct_outputs(outs, given),
            (ValueError, "'max_dist' must be finite and greater than 0", lambda: not (np.isfinite(tfar) and tfar > 0)),
            (ValueError, "array 'azim' has non-finite entries", lambda: not np.isfinite(azim).all()),
            (ValueError, "array 'elev' has non-finite entries", lambda: not np.isfinite(elev).all()),
            (ValueError, "'elev' must lie in [-pi/2, pi/2]", lambda: bool((elev < -half_pi).any() or (elev > half_pi).any())),
            (ValueError, "Vectors in 'vec_north' and/or 'vec_norm' are not normalised",
             lambda: not all(V.unit_vectors(v[None]) for _, v in frames)),
            (ValueError, "array 'observers' has non-finite entries", lambda: not V.all_finite(observers)),
        ))
        self._require_initialised()
        # the four tables of the clause: float64 sin / cos, rounded to float32 once
        azim_sin, azim_cos = np.sin(azim.astype(np.float64)).astype(np.float32), np.cos(azim.astype(np.float64)).astype(np.float32)
        elev_sin, elev_cos = np.sin(elev.astype(np.float64)).astype(np.float32), np.cos(elev.astype(np.float64)).astype(np.float32)
        self._call("hz_terrain_panorama", ptr(observers), observers.shape[0], ptr(azim_sin), ptr(azim_cos), azim.shape[0],
                   ptr(elev_sin), ptr(elev_cos), elev.shape[0], ptr(vec_north), ptr(vec_norm), float(tfar),
                   ptr(dist), ptr(point), ptr(hits))

    # --- additive: any-hit and closest-hit for the caller's own rays ----------------------------------------------------
    def cast(self, origins, directions=None, *, targets=None, max_dist=None, occluded=None, dist=None, point=None,
             order="given"):
        """Traces rays the caller supplies against the whole scene (clause 21): intervisibility of
        point pairs, a sensor's view vector per cell, the pixels of a camera model, a scan pattern.  origins f32[N][3] in
        the scene's frame (that of ``observers`` in ``viewshed``), 1 <= N <= 2**31 - 64, and exactly one of
        ``directions`` f32[N][3], unit vectors (used as given, not normalised) with ``max_dist`` [m] the length of every
        ray (a number, finite and > 0 as float32), or ``targets`` f32[N][3], the far end of a segment (``max_dist`` must
        then be None): the ray runs from the origin to the target and terrain behind the target blocks nothing; a target on
        its origin gives no ray (``occluded`` 0, ``dist`` and ``point`` NaN).  Inputs are NumPy arrays or torch tensors on
        the Terrain's GPU, C-contiguous and finite.  Outputs, any subset, at least one, distinct buffers, every element
        written: ``occluded`` u8[N] 1 if any triangle is hit within the ray, else 0; ``dist`` f32[N] the distance to the
        closest triangle, NaN where nothing is hit (an origin on the surface hits it at 0.0); ``point`` f32[N][3] the hit
        point origin + direction * dist (NaN x 3 where nothing is hit); NumPy or torch tensors on the Terrain's GPU.
        ``occluded`` alone runs an any-hit kernel that stops at the first triangle; it gives the byte the closest-hit
        kernel gives.  ``mask``, ``vec_tilt`` and the inner-domain offsets play no part and refraction is never applied.
        ``order``: "given" traces the rays in the caller's order, "sorted" traces each chunk in an order computed on the
        device (a radix sort of origin and direction codes); the results never depend on it.  The sort costs 0.06 ns per
        ray on an MI355X.  Measured on a 3601 x 3601 tile it paid in one case only: closest-hit rays
        (``dist`` / ``point``) in random order whose origins lie all over the terrain, 20 % faster.  It did not pay for
        ``occluded`` alone (18 % slower), for rays from a handful of origins in any order (33 % slower), or for rays that
        already follow one another in memory the way they do in space.  ``last_stats["num_rays"]`` is the number
        of rays traced: N minus the degenerate segments.  Rays go in chunks: NumPy inputs and outputs are staged on the
        device one chunk at a time and the sort works on one chunk (together at most 256 MiB, plus the sort's histograms), so
        ``last_stats["scratch_bytes"]`` does not grow with N; the copies are not overlapped with the tracing.  The
        finiteness and unit-length checks of inputs given as tensors read reductions back from the GPU: one device
        synchronisation each per call before the launches.  Not offered: a ``max_dist`` per ray, the triangle or cell that
        was hit, one origin shared by all rays, more than one GPU."""
        outs = (("occluded", occluded, 1, np.uint8), ("dist", dist, 1, np.float32), ("point", point, 2, np.float32))
        ends = [(name, v) for name, v in (("directions", directions), ("targets", targets)) if v is not None]
        self._array_arg(origins, 2, "origins")
        for name, v in ends:
            self._array_arg(v, 2, name)
        if max_dist is not None and not V.is_number(max_dist):
            raise TypeError("Argument 'max_dist' has incorrect type (expected a number, got %s)" % type(max_dist).__name__)
        given = self._given_outputs(outs)

        def unit(v):
            if _is_tensor(v):
                return float(((v * v).sum(dim=1) - 1.0).abs().max().item()) <= 1.0e-5
            return V.unit_vectors(v[None])
        with np.errstate(over="ignore"):
            tfar = np.float32(0.0 if max_dist is None else max_dist)         # the ray length the kernel sees
        n = lambda: origins.shape[0]                                          # noqa: E731
        V.run((
            (ValueError, "exactly one of 'directions' and 'targets' must be given", lambda: len(ends) != 1),
            (ValueError, "'max_dist' must be given with 'directions'", lambda: directions is not None and max_dist is None),
            (ValueError, "'max_dist' must be None with 'targets'", lambda: targets is not None and max_dist is not None),
            V.some_output_given(outs, given),
            (ValueError, "'order' must be 'given' or 'sorted'", lambda: not isinstance(order, str) or order not in ("given", "sorted")),
            (ValueError, "array 'origins' has incorrect shape", lambda: origins.shape[1] != 3 or n() < 1),
            (ValueError, "'origins' must not have more than 2**31 - 64 rays", lambda: n() > 2 ** 31 - 64),
            (ValueError, "array '%s' has incorrect shape" % ends[0][0] if ends else "",
             lambda: tuple(ends[0][1].shape) != (n(), 3)),
            (ValueError, "array 'occluded' has incorrect shape", lambda: occluded is not None and tuple(occluded.shape) != (n(),)),
            (ValueError, "array 'dist' has incorrect shape", lambda: dist is not None and tuple(dist.shape) != (n(),)),
            (ValueError, "array 'point' has incorrect shape", lambda: point is not None and tuple(point.shape) != (n(), 3)),
            V.all_contiguous(lambda: [origins, ends[0][1]] + given),
            V.distinct_outputs(outs, given),
            (ValueError, "'max_dist' must be finite and greater than 0",
             lambda: directions is not None and not (np.isfinite(tfar) and tfar > 0)),
            (ValueError, "array 'origins' has non-finite entries", lambda: not V.all_finite(origins)),
            (ValueError, "array '%s' has non-finite entries" % ends[0][0] if ends else "", lambda: not V.all_finite(ends[0][1])),
            (ValueError, "Vectors in 'directions' are not normalised", lambda: directions is not None and not unit(directions)),
        ))
        self._require_initialised()
        self._call("hz_terrain_cast", ptr(origins), ptr(directions), ptr(targets), origins.shape[0], float(tfar),
                   1 if order == "sorted" else 0, ptr(occluded), ptr(dist), ptr(point))

    # --- additive: the lowest target height in sight, per observer and cell --------------------------------------------
    def sight_height(self, observers, heights, *, height=None, lowest=None, cells_reached=None, max_dist=None):
        """How high above each cell a target must be to have a free line of sight to each point of observers f32[S][3]
        (as in ``viewshed``), out of the table heights f32[n] [m] (1 <= n <= 65535, finite, strictly increasing,
        heights[0] >= 0.005; a NumPy array, e.g. from ``sight_heights``): the smallest entry whose point above the surface
        along ``vec_norm`` is in sight, found by asking for the top of the table, then its bottom, then bisecting
        (clause 19) -- at most 2 + ceil(log2(n - 1)) rays per observer and cell instead of one
        ``viewshed`` call per height.  +inf where not even the top of the table is in sight or the cell is farther than
        ``max_dist`` [m] (None or > 0; judged at heights[0]); NaN where masked.  No facing test (an elevated target is
        not a surface); refraction is never applied.  Where visibility is not monotone in the height the bisection
        returns one visible entry above a blocked one, not necessarily the first.  Outputs, any subset, at least one:
        ``height`` f32[S][y][x] the results, ``lowest`` f32[y][x] their minimum over the observers, ``cells_reached``
        i64[S] the cells with a finite result per observer; NumPy or torch tensors on the Terrain's GPU.
        ``last_stats["num_rays"]`` is the number of rays traced; ``last_stats["scratch_bytes"]`` does not grow with S."""
        outs = (("height", height, 3, np.float32), ("lowest", lowest, 2, np.float32),
                ("cells_reached", cells_reached, 1, np.int64))
        self._array_arg(observers, 2, "observers")
        if not isinstance(heights, np.ndarray):
            raise TypeError("Argument 'heights' has incorrect type (expected numpy.ndarray, got %s)" % type(heights).__name__)
        _typed(heights, np.float32, 1, "heights")
        given = self._given_outputs(outs)
        if max_dist is not None and not V.is_number(max_dist):
            raise TypeError("Argument 'max_dist' has incorrect type (expected a number or None, got %s)" % type(max_dist).__name__)
        V.run((
            V.some_output_given(outs, given),
            (ValueError, "array 'observers' has incorrect shape", lambda: observers.shape[1] != 3 or observers.shape[0] < 1),
            (ValueError, "array 'heights' must have 1 to 65535 entries", lambda: not 1 <= heights.shape[0] <= 65535),
            (ValueError, "array 'height' has incorrect shape",
             lambda: height is not None and height.shape[0] != observers.shape[0]),
            (ValueError, "array 'cells_reached' has incorrect shape",
             lambda: cells_reached is not None and cells_reached.shape[0] != observers.shape[0]),
            V.all_contiguous(lambda: [observers, heights] + given),
            V.distinct_outputs(outs, given),
            (ValueError, "array 'heights' has non-finite entries", lambda: not np.isfinite(heights).all()),
            (ValueError, "'heights' must start at 0.005 m or above", lambda: not heights[0] >= np.float32(0.005)),
            (ValueError, "'heights' must be strictly increasing", lambda: not (heights[1:] > heights[:-1]).all()),
            (ValueError, "'max_dist' must be None or greater than 0", lambda: max_dist is not None and not np.float32(max_dist) > 0),
            (ValueError, "array 'observers' has non-finite entries", lambda: not V.all_finite(observers)),
        ))
        for name, buf in (("height", height), ("lowest", lowest)):
            if buf is not None:
                self._check_out(buf, name)
        self._require_initialised()
        self._call("hz_terrain_sight_height", ptr(observers), observers.shape[0], ptr(heights), heights.shape[0],
                   0.0 if max_dist is None else float(max_dist), ptr(height), ptr(lowest), ptr(cells_reached))


def sight_heights(height_max, height_acc=0.25, height_min=0.05):
    """A height table for ``Terrain.sight_height``: float32 of height_min + k * height_acc, k = 0 ... K, formed in float64, with
    K = ceil((height_max - height_min) / height_acc): the last entry is the first at or above height_max (it exceeds it by less
    than one step).  ValueError if the table would have more than 65535 entries, if it would start below 0.005 m, or if
    rounding to float32 makes two neighbours equal (a step too fine for the heights)."""
    for name, v in (("height_max", height_max), ("height_acc", height_acc), ("height_min", height_min)):
        if not V.is_number(v):
            raise TypeError("Argument '%s' has incorrect type (expected a number, got %s)" % (name, type(v).__name__))
    lo, hi, acc = np.float64(height_min), np.float64(height_max), np.float64(height_acc)
    if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(acc)):
        raise ValueError("'height_max', 'height_acc' and 'height_min' must be finite")
    if not acc > 0.0:
        raise ValueError("'height_acc' must be greater than 0")
    if not np.float32(lo) >= np.float32(0.005):
        raise ValueError("'height_min' must be at least 0.005 m")
    if not hi >= lo:
        raise ValueError("'height_max' must not be below 'height_min'")
    steps = np.ceil((hi - lo) / acc)
    if steps + 1 > 65535:
        raise ValueError("the table would have %d entries (at most 65535)" % (int(steps) + 1))
    table = (lo + np.arange(int(steps) + 1, dtype=np.float64) * acc).astype(np.float32)
    if not (table[1:] > table[:-1]).all():
        raise ValueError("'height_acc' is too small for float32: neighbouring entries are equal")
    return table


def _is_tensor(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def gridded_azimuths(azim_num):
    """The azimuth array ``horizon_gridded`` returns for ``azim_num`` directions: float32 of 2 pi k / azim_num."""
    azim = np.empty(azim_num, dtype=np.float32)
    for i in range(azim_num):
        azim[i] = ((2 * np.pi) / azim_num * i)
    return azim


class HorizonTerrain:
    """``Terrain``'s answers from a stored horizon instead of a ray (additive, not in the reference): a cell is
    terrain-shaded when the sun's elevation in the cell's frame is below the horizon ``hori`` of ``horizon_gridded``,
    interpolated linearly at the sun's azimuth (clause 10).  No scene and no BVH; the self-shading and
    ``ang_max`` tests, the shadow codes, the ``sw_dir_cor`` formula and the sums of ``accumulate`` are ``Terrain``'s, and so
    are the method names and signatures.  Atmospheric refraction is switched on by ``refraction(elevation)`` after
    ``initialise`` (a method of its own: ``initialise`` keeps its arguments); every method then answers for the refracted
    sun, with ``Terrain``'s ``refrac_cor=True`` set-up word for word (clause 13)."""
    _NAME = "HorizonTerrain"            # in messages

    def __init__(self, *, device=0):
        self._h = C.c_void_p()
        self._shape = None
        self._hori = None
        self._refrac = False
        self.device = device
        self.last_stats = None
        _lib.check(_lib.lib().hz_horizon_terrain_create(device, C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().hz_horizon_terrain_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _typed_hori(self, hori):
        """``hori``: a NumPy array, or a torch tensor on the object's GPU (borrowed: the object holds a reference)."""
        if isinstance(hori, np.ndarray):
            _typed(hori, np.float32, 3, "hori")
            return
        if not hasattr(hori, "data_ptr"):
            raise TypeError("Argument 'hori' has incorrect type (expected numpy.ndarray or torch.Tensor, got %s)"
                            % type(hori).__name__)
        if hori.dim() != 3:
            raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % hori.dim())
        if str(hori.dtype).split(".")[-1] != "float32":
            raise ValueError("Buffer dtype mismatch, expected 'float32' but got '%s'" % hori.dtype)
        if hori.device.type != "cuda" or hori.device.index != self.device:
            raise ValueError("tensor 'hori' is not on the HorizonTerrain's device (cuda:%d)" % self.device)

    def initialise(self, azim, hori, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                   vec_tilt, vec_norm, vec_north, surf_enl_fac, mask,
                   sw_dir_cor_fill=np.nan, ang_max=89.0):
        """Initialise with the horizon ``hori`` f32 (y, x, azim_num) [radian] and ``azim`` as ``horizon_gridded`` returns
        them (``azim[k] = 2 pi k / azim_num`` is the only layout supported; azim_num >= 1), the DEM vertices and the
        per-cell arrays of ``Terrain.initialise`` plus ``vec_north``.  ``hori`` is a NumPy array (copied to the GPU) or a
        torch tensor on the object's GPU (borrowed: the object holds a reference, the data must not change while it is in
        use); the other arrays are NumPy and are copied.  Atmospheric refraction is off afterwards; ``refraction(elevation)``
        switches it on."""
        self._initialise(False, azim, hori, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                         vec_tilt, vec_norm, vec_north, surf_enl_fac, mask, sw_dir_cor_fill, ang_max)

    def initialise_azim_major(self, azim, hori, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                              vec_tilt, vec_norm, vec_north, surf_enl_fac, mask,
                              sw_dir_cor_fill=np.nan, ang_max=89.0):
        """``initialise`` with the horizon in the azimuth-major layout: ``hori`` f32 (azim_num, y, x), what
        ``horizon_gridded(layout="azim_major")`` returns or ``horizon.to_azim_major`` makes of a cell-major horizon (NumPy:
        copied; torch tensor on the object's GPU: borrowed).  Every other argument and every check is ``initialise``'s,
        and so is every result of the methods, bit for bit; a wave's look-up is two loads of consecutive words per position
        instead of one line per lane, with atmospheric refraction (``refraction``) or without.  (A method of its own:
        ``initialise`` keeps exactly ``Terrain``-style arguments.)"""
        self._initialise(True, azim, hori, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                         vec_tilt, vec_norm, vec_north, surf_enl_fac, mask, sw_dir_cor_fill, ang_max)

    def initialise_q16(self, azim, hori_q, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                       vec_tilt, vec_norm, vec_north, surf_enl_fac, mask,
                       sw_dir_cor_fill=np.nan, ang_max=89.0, *, layout="cell_major"):
        """``initialise`` with the horizon as 16-bit codes (clause 15): ``hori_q`` uint16 (y, x,
        azim_num), or (azim_num, y, x) with ``layout="azim_major"`` -- what ``horizon_gridded(hori_dtype="uint16")`` returns
        or ``horizon.quantise`` makes of a float32 horizon (NumPy: copied; torch tensor on the object's GPU, ``torch.uint16``
        or ``torch.int16`` with the same bits: borrowed).  Half the bytes of the float32 horizon in HBM.  Every method then
        gives, word for word, what it gives on the float32 horizon ``horizon.dequantise(hori_q)`` in the same layout;
        ``sw_dir_cor_coarse`` always takes the two-pass route.  Every other argument and check is ``initialise``'s.  (A method
        of its own: ``initialise`` and ``initialise_azim_major`` keep taking float32 only.)"""
        from .horizon import check_layout
        self._initialise(check_layout(layout), azim, hori_q, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                         vec_tilt, vec_norm, vec_north, surf_enl_fac, mask, sw_dir_cor_fill, ang_max, q16=True)

    def _typed_hori_q(self, hori_q):
        """``_typed_hori`` for codes: uint16, for a tensor also int16."""
        if isinstance(hori_q, np.ndarray):
            _typed(hori_q, np.uint16, 3, "hori_q")
            return
        if not hasattr(hori_q, "data_ptr"):
            raise TypeError("Argument 'hori_q' has incorrect type (expected numpy.ndarray or torch.Tensor, got %s)"
                            % type(hori_q).__name__)
        if hori_q.dim() != 3:
            raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % hori_q.dim())
        if str(hori_q.dtype).split(".")[-1] not in ("uint16", "int16"):
            raise ValueError("Buffer dtype mismatch, expected 'uint16' but got '%s'" % hori_q.dtype)
        if hori_q.device.type != "cuda" or hori_q.device.index != self.device:
            raise ValueError("tensor 'hori_q' is not on the HorizonTerrain's device (cuda:%d)" % self.device)

    def _initialise(self, planes, azim, hori, vert_grid, dem_dim_0, dem_dim_1, offset_0, offset_1,
                    vec_tilt, vec_norm, vec_north, surf_enl_fac, mask, sw_dir_cor_fill, ang_max, q16=False):
        _typed(azim, np.float32, 1, "azim")
        (self._typed_hori_q if q16 else self._typed_hori)(hori)
        _typed(vert_grid, np.float32, 1, "vert_grid")
        _typed(vec_tilt, np.float32, 3, "vec_tilt")
        _typed(vec_norm, np.float32, 3, "vec_norm")
        _typed(vec_north, np.float32, 3, "vec_north")
        _typed(surf_enl_fac, np.float32, 2, "surf_enl_fac")
        _typed(mask, np.uint8, 2, "mask")

        vectors = (vec_tilt, vec_norm, vec_north)
        cells, num = (tuple(hori.shape[1:]), hori.shape[0]) if planes else (tuple(hori.shape[:2]), hori.shape[2])
        host = [a for a in (azim, hori, vert_grid, vec_tilt, vec_norm, vec_north, surf_enl_fac, mask) if not _is_tensor(a)]
        V.run((
            (ValueError, "inconsistency between input arguments 'vert_grid', 'dem_dim_0' and 'dem_dim_1'",
             lambda: not V.fits_grid(len(vert_grid), dem_dim_0, dem_dim_1)),
            (ValueError, "inconsistency between input arguments 'dem_dim_0', 'dem_dim_1', 'offset_0', 'offset_1' and 'vec_norm'",
             lambda: not V.window_inside(offset_0, offset_1, vec_tilt.shape, dem_dim_0, dem_dim_1)),
            (ValueError, "Inconsistent/incorrect shape of 'vec_tilt', 'vec_norm' and/or 'vec_north'",
             lambda: not V.same_leading_shape(vectors, 3, 3) or vec_tilt.shape[2] != 3),
            (ValueError, "Inconsistent/incorrect shape of 'surf_enl_fac' and/or 'mask'",
             lambda: not V.same_leading_shape((vec_tilt[..., 0], surf_enl_fac, mask), 2, 2)),
            (ValueError, "Inconsistent/incorrect shape of '%s'" % ("hori_q" if q16 else "hori"),
             lambda: cells != vec_tilt.shape[:2] or num < 1),
            (ValueError, "'azim' is not the azimuth array of horizon_gridded",
             lambda: azim.shape[0] != num or not np.array_equal(azim, gridded_azimuths(num))),
            (ValueError, "not all input arrays are C-contiguous",
             lambda: not all(a.flags["C_CONTIGUOUS"] for a in host) or (_is_tensor(hori) and not hori.is_contiguous())),
            (ValueError, "Vectors in 'vec_tilt', 'vec_norm' and/or 'vec_north' are not normalised",
             lambda: not all(V.unit_vectors(v) for v in vectors)),
            (TypeError, "'ang_max' must be in the range [85.0, 89.99]", lambda: ang_max < 85.0 or ang_max > 89.99),
            (ValueError, V.MSG_DIM_LIMIT, lambda: max(dem_dim_0, dem_dim_1) > V.DIM_LIMIT),
        ))

        st = hz_stats()
        self._shape = None
        self._refrac = False                                 # the library drops the factor with the old arrays
        L = _lib.lib()
        entry = L.hz_horizon_terrain_initialise_q16 if q16 else \
            (L.hz_horizon_terrain_initialise_planes if planes else L.hz_horizon_terrain_initialise)
        _lib.check(entry(
            self._h, ptr(hori), num, *((int(planes),) if q16 else ()), ptr(vert_grid), dem_dim_0, dem_dim_1, offset_0, offset_1,
            ptr(vec_tilt), ptr(vec_norm), ptr(vec_north), vec_tilt.shape[0], vec_tilt.shape[1],
            ptr(surf_enl_fac), ptr(mask), sw_dir_cor_fill, ang_max, C.byref(st)))
        self._hori = hori if _is_tensor(hori) else None      # keep a borrowed horizon alive
        self._shape = (vec_tilt.shape[0], vec_tilt.shape[1])
        self.last_stats = st.as_dict()

    def refraction(self, elevation):
        """Switch atmospheric refraction on or off for every later call (clause 13).  ``elevation``
        f32 (y, x) [m]: the orthometric elevation of the inner-domain cells, ``Terrain.initialise``'s ``elevation`` (a
        C-contiguous NumPy array, copied; no range check, as there); ``None`` switches it off.  With it, ``shadow``,
        ``sw_dir_cor``, the batch forms, ``accumulate`` and ``sw_dir_cor_coarse`` answer for the sun as the atmosphere bends
        it over each cell -- ``Terrain``'s ``refrac_cor=True`` -- on both horizon layouts.  ``initialise``,
        ``initialise_azim_major`` and ``initialise_q16`` switch it off again."""
        if elevation is not None:
            _typed(elevation, np.float32, 2, "elevation")
        self._require_initialised()
        if elevation is not None:
            if tuple(elevation.shape) != self._shape:
                raise ValueError("array 'elevation' has incorrect shape")
            if not elevation.flags["C_CONTIGUOUS"]:
                raise ValueError("array 'elevation' is not C-contiguous")
        st = hz_stats()
        self._refrac = False
        _lib.check(_lib.lib().hz_horizon_terrain_refraction(self._h, ptr(elevation), C.byref(st)))
        self._refrac = elevation is not None
        self.last_stats = st.as_dict()

    @property
    def refrac_cor(self):
        """Whether the methods answer for the refracted sun (``refraction``)."""
        return bool(getattr(self, "_refrac", False))

    _batch_out = staticmethod(Terrain._batch_out)
    _array_arg = Terrain._array_arg

    _require_initialised = Terrain._require_initialised
    _call = Terrain._call
    _check_out = Terrain._check_out

    def _run(self, sun_positions, weights, num_sun, **outs):
        out = _lib.hz_horisun_out(**{k: ptr(v) for k, v in outs.items()})
        self._call("hz_horizon_terrain_run", ptr(sun_positions), ptr(weights), num_sun, C.byref(out))

    def shadow(self, sun_position, shadow_buffer):
        """Compute shadow mask for specified sun position
        (0: illuminated, 1: self-shaded, 2: terrain-shaded, 3: masked)."""
        _typed(sun_position, np.float32, 1, "sun_position")
        _typed(shadow_buffer, np.uint8, 2, "shadow_buffer")
        if (sun_position.ndim != 1) or (sun_position.size != 3):
            raise ValueError("array 'sun_position' has incorrect shape")
        if not shadow_buffer.flags["C_CONTIGUOUS"]:
            raise ValueError("array 'shadow_buffer' is not C-contiguous")
        self._check_out(shadow_buffer, "shadow_buffer")
        self._run(np.ascontiguousarray(sun_position), None, 1, shadow=shadow_buffer)

    def sw_dir_cor(self, sun_position, sw_dir_cor_buffer):
        """Compute shortwave correction factor for specified sun position."""
        _typed(sun_position, np.float32, 1, "sun_position")
        _typed(sw_dir_cor_buffer, np.float32, 2, "sw_dir_cor_buffer")
        if (sun_position.ndim != 1) or (sun_position.size != 3):
            raise ValueError("array 'sun_position' has incorrect shape")
        if not sw_dir_cor_buffer.flags["C_CONTIGUOUS"]:
            raise ValueError("array 'sw_dir_cor_buffer' is not C-contiguous")
        self._check_out(sw_dir_cor_buffer, "sw_dir_cor_buffer")
        self._run(np.ascontiguousarray(sun_position), None, 1, sw_dir_cor=sw_dir_cor_buffer)

    def shadow_batch(self, sun_positions, shadow_buffers):
        """``shadow`` for sun_positions f32[num][3] -> shadow_buffers u8[num][y][x] (NumPy or torch/HBM)."""
        _typed(sun_positions, np.float32, 2, "sun_positions")
        self._batch_out(shadow_buffers, np.uint8, "shadow_buffers")
        if sun_positions.shape[1] != 3 or sun_positions.shape[0] < 1 or shadow_buffers.shape[0] != sun_positions.shape[0]:
            raise ValueError("array 'sun_positions' has incorrect shape")
        self._check_out(shadow_buffers, "shadow_buffers")
        self._run(np.ascontiguousarray(sun_positions), None, sun_positions.shape[0], shadow=shadow_buffers)

    def sw_dir_cor_batch(self, sun_positions, sw_dir_cor_buffers):
        """``sw_dir_cor`` for sun_positions f32[num][3] -> sw_dir_cor_buffers f32[num][y][x] (NumPy or torch/HBM)."""
        _typed(sun_positions, np.float32, 2, "sun_positions")
        self._batch_out(sw_dir_cor_buffers, np.float32, "sw_dir_cor_buffers")
        if sun_positions.shape[1] != 3 or sun_positions.shape[0] < 1 or sw_dir_cor_buffers.shape[0] != sun_positions.shape[0]:
            raise ValueError("array 'sun_positions' has incorrect shape")
        self._check_out(sw_dir_cor_buffers, "sw_dir_cor_buffers")
        self._run(np.ascontiguousarray(sun_positions), None, sun_positions.shape[0], sw_dir_cor=sw_dir_cor_buffers)

    def accumulate(self, sun_positions, weights=None, *, sw_dir_cor_sum=None, sunlit_sum=None,
                   shadow_buffers=None, sw_dir_cor_buffers=None):
        """``Terrain.accumulate`` from the horizon: ``sw_dir_cor_sum`` = sum of weights[s] * sw_dir_cor(sun_positions[s]) and
        ``sunlit_sum`` = sum of weights[s] over the positions for which shadow() gives 0, per cell, accumulated in float64
        in ascending s and rounded to float32 once; masked cells get ``sw_dir_cor_fill``.  sun_positions f32[S][3] (S >= 1),
        weights f32[S] (None: ones); outputs f32[y][x], NumPy or torch tensors on the object's GPU; at least one.  The sums
        stay in registers: device memory besides the buffers does not grow with S (``last_stats["scratch_bytes"]``).
        ``shadow_buffers`` u8[S][y][x] and ``sw_dir_cor_buffers`` f32[S][y][x] (keyword only, not in ``Terrain``; NumPy or
        torch/HBM) also take the per-position maps of the same pass."""
        outs = (("sw_dir_cor_sum", sw_dir_cor_sum), ("sunlit_sum", sunlit_sum))
        _accumulate_types(self, sun_positions, weights, outs)
        if shadow_buffers is not None:
            self._batch_out(shadow_buffers, np.uint8, "shadow_buffers")
        if sw_dir_cor_buffers is not None:
            self._batch_out(sw_dir_cor_buffers, np.float32, "sw_dir_cor_buffers")
        maps = [(n, b) for n, b in (("shadow_buffers", shadow_buffers), ("sw_dir_cor_buffers", sw_dir_cor_buffers))
                if b is not None]
        V.run(_accumulate_checks(sun_positions, weights, outs) + (
            (ValueError, "array 'shadow_buffers' / 'sw_dir_cor_buffers' has incorrect shape",
             lambda: any(b.shape[0] != sun_positions.shape[0] for _, b in maps)),
        ))
        for name, buf in tuple(outs) + tuple(maps):
            if buf is not None:
                self._check_out(buf, name)
        self._run(sun_positions, weights, sun_positions.shape[0], sw_dir_cor_sum=sw_dir_cor_sum, sunlit_sum=sunlit_sum,
                  shadow=shadow_buffers, sw_dir_cor=sw_dir_cor_buffers)

    _pixel_per_gc = staticmethod(Terrain._pixel_per_gc)

    def sw_dir_cor_coarse(self, sun_positions, pixel_per_gc, *, f_cor=None, sunlit_frac=None):
        """``Terrain.sw_dir_cor_coarse`` from the horizon (clause 12): per sun position of sun_positions
        f32[S][3] (S >= 1), means over blocks of P0 x P1 cells of the inner domain (``pixel_per_gc``: an int P or a pair
        (P0, P1) that divide its shape), without a map per position: ``f_cor[s][I][J]`` = the mean of
        sw_dir_cor(sun_positions[s]) and ``sunlit_frac[s][I][J]`` = the fraction of cells for which shadow() gives 0, both
        over the unmasked cells of the block.  The sum is a float64 accumulator over the block's unmasked cells in row-major
        order, divided by their number in float64 and rounded to float32 once; a block without an unmasked cell gets
        ``sw_dir_cor_fill``.  Outputs f32[S][gy][gx], NumPy or torch tensors on the object's GPU; at least one.  Both horizon
        layouts give the same words.  Device memory besides the outputs does not grow with S
        (``last_stats["scratch_bytes"]``)."""
        _sw_dir_cor_coarse(self, "hz_horizon_terrain_sw_dir_cor_coarse", sun_positions, pixel_per_gc, f_cor, sunlit_frac)

    def sun_times(self, sun_positions, times, *, sunrise=None, sunset=None, duration=None, intervals=None):
        """Maps over a sun track (clause 14): sun_positions f32[S][3] (S >= 1) at the ``times``
        f64[S] (a NumPy array: finite, strictly increasing, in the caller's unit).  Per cell: ``sunrise`` = the time the sun
        first clears terrain and surface, ``sunset`` = the time it last does, ``duration`` = the sunlit time in between,
        ``intervals`` = the number of separate sunlit spells (a peak that interrupts the sun gives two).  A position is sunlit
        exactly where ``shadow()`` gives 0.  Between two positions with different states the crossing time is interpolated
        linearly from the sun's clearances g = min(alpha - h, asin(dot_ts)) [rad] at the two, so a coarse track gives event
        times far finer than its step; a cell lit at the first or last position gets ``times[0]`` / ``times[-1]``.  Cells
        never lit get NaN, NaN, 0.0 and 0; masked cells ``sw_dir_cor_fill`` and -1.  Outputs f32[y][x] (``intervals``:
        i32[y][x]), NumPy or torch tensors on the object's GPU; any subset, at least one.  Works with ``refraction`` on and in
        both horizon layouts (the same words).  Device memory besides the buffers is 44 B per cell when the track spans
        several launches and does not grow with S (``last_stats["scratch_bytes"]``).  ``Terrain`` (the ray path) has no such
        method: a ray says whether the sun is hidden, not by how much it clears, so there is nothing to interpolate."""
        outs = (("sunrise", sunrise, np.float32), ("sunset", sunset, np.float32), ("duration", duration, np.float32),
                ("intervals", intervals, np.int32))
        self._array_arg(sun_positions, 2, "sun_positions")
        _typed(times, np.float64, 1, "times")
        for name, buf, dtype in outs:
            if buf is not None:
                self._array_arg(buf, 2, name, dtype, self._NAME)
        self._require_initialised()
        given = [(name, buf) for name, buf, _ in outs if buf is not None]
        V.run((
            (ValueError, "at least one of 'sunrise', 'sunset', 'duration' and 'intervals' must be given", lambda: not given),
            (ValueError, "array 'sun_positions' has incorrect shape",
             lambda: sun_positions.shape[1] != 3 or sun_positions.shape[0] < 1),
            (ValueError, "array 'times' has incorrect shape", lambda: times.shape[0] != sun_positions.shape[0]),
        ) + tuple(
            (ValueError, "array '%s' has incorrect shape" % name, lambda buf=buf: tuple(buf.shape) != self._shape)
            for name, buf in given
        ) + (
            (ValueError, "not all input arrays are C-contiguous",
             lambda: not all(_contiguous(a) for a in [sun_positions, times] + [buf for _, buf in given])),
            (ValueError, "'sunrise', 'sunset', 'duration' and 'intervals' must be different arrays",
             lambda: len({ptr(buf) for _, buf in given}) != len(given)),
            (ValueError, "'times' must be finite and strictly increasing",
             lambda: not (np.isfinite(times).all() and (np.diff(times) > 0.0).all())),
        ))
        out = _lib.hz_suntimes_out(**{name: ptr(buf) for name, buf in given})
        self._call("hz_horizon_terrain_sun_times", ptr(sun_positions), ptr(times), sun_positions.shape[0], C.byref(out))
