"""horayzon.topo_param on MI355X: the reductions of a horizon array (sky view factor, visible sky
fraction, topographic openness; reference: horayzon/topo_param.pyx:377-603, and all three in one
pass: topo_parameters) and the slope computations (:16-372)."""
import numpy as np

from . import _lib
from ._lib import ptr


def _cell_shape(hori, layout):
    """(planes?, (y, x), azim_num) of a 3-D horizon in ``layout`` ("cell_major": (y, x, azim); "azim_major": (azim, y, x))."""
    from .horizon import check_layout
    planes = check_layout(layout)
    if not planes:
        return False, tuple(hori.shape[:2]), hori.shape[2]
    if hori.ndim != 3:
        raise ValueError("Inconsistent/incorrect shapes of input arrays")
    return True, tuple(hori.shape[1:]), hori.shape[0]


def _is_tensor(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _dtype_name(a):
    return str(a.dtype).split(".")[-1]          # "float32" of np.float32 and of torch.float32


def _contiguous(a, name, copy):
    """``a`` C-contiguous: small arrays (azim, vec_tilt; ``copy``) are copied if need be, a horizon never is --
    np.ascontiguousarray of planes would silently copy 18 GB, and a tensor horizon stays where it is."""
    if _is_tensor(a):
        if a.is_contiguous():
            return a
        if copy:
            return a.contiguous()
    elif copy or a.flags["C_CONTIGUOUS"]:
        return np.ascontiguousarray(a)
    raise ValueError("array '%s' is not C-contiguous" % name)


TOPO_NAMES = ("svf", "vsf", "openness")
# a single output on a cell-major float32 horizon keeps its own entry point (the exports stay exercised)
_SINGLE = {"svf": "hz_sky_view_factor", "vsf": "hz_visible_sky_fraction", "openness": "hz_topographic_openness"}


def _reduce(names, azim, hori, vec_tilt, device, layout, single=False):
    """``{name: float32 (y, x)}`` for the ``names`` out of TOPO_NAMES: the reference's shape and dtype checks
    (topo_param.pyx:398-404, :486-492, :565-569), the contiguity handling and the library call.  ``single``: ``names`` is
    one name, and a cell-major float32 horizon goes to that output's own entry point.  ``hori`` is float32 or the 16-bit
    code (uint16; a tensor may carry the same bits as int16), a NumPy array or a torch tensor on a GPU; with a tensor
    ``hori`` the other arrays may be tensors on that GPU too and the maps are tensors there."""
    tilted = "svf" in names or "vsf" in names
    tensor = _is_tensor(hori)
    planes, cells, num = _cell_shape(hori, layout)
    cells = tuple(cells)
    codes = ("uint16", "int16") if tensor else ("uint16",)
    if tilted:
        if (len(azim) != num) or (cells != tuple(vec_tilt.shape[:2]))\
                or (vec_tilt.shape[2] != 3):
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
        if ((_dtype_name(azim) != "float32") or (_dtype_name(hori) not in ("float32",) + codes)
                or (_dtype_name(vec_tilt) != "float32")):
            raise ValueError("Input array(s) has/have incorrect data type(s)")
        if len(azim) < 2:   # azim[1] - azim[0] is read (topo_param.pyx:433, :520): out of bounds in the reference
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
    else:
        if len(azim) != num:
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
        if (_dtype_name(azim) != "float32") or (_dtype_name(hori) not in ("float32",) + codes):
            raise ValueError("Input array(s) has/have incorrect data type(s)")
        vec_tilt = None
    q16 = _dtype_name(hori) != "float32"
    others = [("azim", azim)] + ([("vec_tilt", vec_tilt)] if tilted else [])
    if tensor:
        if hori.device.type != "cuda":
            raise ValueError("tensor 'hori' is not on a GPU")
        for name, a in others:
            if _is_tensor(a) and a.device != hori.device:
                raise ValueError("tensor '%s' is not on the device of 'hori'" % name)
        device = hori.device.index
    elif any(_is_tensor(a) for _, a in others):
        raise ValueError("a tensor 'azim' or 'vec_tilt' needs a tensor 'hori'")
    azim = _contiguous(azim, "azim", True)
    if tilted:
        vec_tilt = _contiguous(vec_tilt, "vec_tilt", True)
    hori = _contiguous(hori, "hori", not planes and not tensor)
    if tensor:
        import torch
        out = {n: torch.empty(cells, dtype=torch.float32, device=hori.device) for n in TOPO_NAMES if n in names}
        torch.cuda.synchronize(hori.device)       # the library works on a stream of its own
    else:
        out = {n: np.empty(cells, dtype=np.float32) for n in TOPO_NAMES if n in names}
    L = _lib.lib()
    maps = (ptr(out.get("svf")), ptr(out.get("vsf")), ptr(out.get("openness")))
    if q16:
        _lib.check(L.hz_topo_params_q16(ptr(azim), ptr(hori), int(planes), ptr(vec_tilt), cells[0], cells[1], num, *maps, device))
    elif single and not planes:
        tilt_arg = (ptr(vec_tilt),) if tilted else ()
        _lib.check(getattr(L, _SINGLE[names[0]])(ptr(azim), ptr(hori), *tilt_arg, cells[0], cells[1], num,
                                                 ptr(out[names[0]]), device))
    else:
        _lib.check((L.hz_topo_params_planes if planes else L.hz_topo_params)(
            ptr(azim), ptr(hori), ptr(vec_tilt), cells[0], cells[1], num, *maps, device))
    return out


def sky_view_factor(azim, hori, vec_tilt, *, device=0, layout="cell_major"):
    """Sky view factor (SVF) computation.

    Same arguments, checks and result as the reference
    (topo_param.pyx:377-409): azim float32 (azim), hori float32 (y, x, azim)
    [radian], vec_tilt float32 (y, x, 3); returns svf float32 (y, x).  With
    ``layout="azim_major"`` (not in the reference) hori is float32 (azim, y, x), C-contiguous; the result is the
    same, bit for bit.

    ``hori`` may also hold the 16-bit horizon code (uint16, ``horizon.quantise`` / ``hori_dtype="uint16"``) in either
    layout: the codes are reduced as they are, without a float32 copy, and the result is, word for word, that of
    ``dequantise(hori)`` (``Q16_NAN`` behaves as a NaN horizon).  And ``hori`` may be a C-contiguous torch tensor on a GPU
    (float32, uint16, or int16 carrying the code's bits), which is never copied to the host; ``azim`` and ``vec_tilt`` may
    then each be NumPy or a tensor on that GPU, and the result is a float32 tensor there."""
    return _reduce(["svf"], azim, hori, vec_tilt, device, layout, single=True)["svf"]


def visible_sky_fraction(azim, hori, vec_tilt, *, device=0, layout="cell_major"):
    """Visible sky fraction (solid angle of the visible sky); arguments, checks and result as the
    reference (topo_param.pyx:465-496); ``layout``, 16-bit codes and GPU tensors as in ``sky_view_factor``."""
    return _reduce(["vsf"], azim, hori, vec_tilt, device, layout, single=True)["vsf"]


def topographic_openness(azim, hori, *, device=0, layout="cell_major"):
    """Positive topographic openness (Yokoyama et al. 2002) [radian]; arguments, checks and result as
    the reference (topo_param.pyx:548-574); ``layout``, 16-bit codes and GPU tensors as in ``sky_view_factor``."""
    return _reduce(["openness"], azim, hori, None, device, layout, single=True)["openness"]


def topo_parameters(azim, hori, vec_tilt=None, which=TOPO_NAMES, *, device=0, layout="cell_major"):
    """Any of the three reductions above -- sky view factor ("svf"), visible sky fraction ("vsf"),
    positive topographic openness ("openness") -- from ONE pass over the horizon array
    (hz_topo_params).  Arguments and checks as the single-output functions (topo_param.pyx:398-404,
    :486-492, :565-569); ``vec_tilt`` is needed for "svf" and "vsf" only.  Returns
    ``{name: float32 (y, x)}``, each map bit-identical to the single-output function's.  ``layout="azim_major"``: hori is
    float32 (azim, y, x), C-contiguous (hz_topo_params_planes); the maps are the same, bit for bit.  16-bit codes and
    GPU tensors as in ``sky_view_factor`` (hz_topo_params_q16)."""
    names = [which] if isinstance(which, str) else list(which)
    if not names:
        raise ValueError("'which' is empty")
    unknown = [n for n in names if n not in TOPO_NAMES]
    if unknown:
        raise ValueError("unknown name(s) in 'which': %r (choose from %r)" % (unknown, TOPO_NAMES))
    if ("svf" in names or "vsf" in names) and vec_tilt is None:
        raise ValueError("'svf' and 'vsf' need 'vec_tilt'")
    return _reduce(names, azim, hori, vec_tilt, device, layout)


def _slope(which, x, y, z, rot_mat, output_rot, device):
    # Check arguments (topo_param.pyx:59-72 / :262-277)
    if (x.shape != y.shape) or (y.shape != z.shape):
        raise ValueError("Inconsistent shapes / number of dimensions of "
                         + "input arrays")
    if ((x.dtype != "float32") or (y.dtype != "float32")
            or (z.dtype != "float32")):
        raise ValueError("Input array(s) has/have incorrect data type(s)")
    if which == 1 and output_rot and (rot_mat is None):
        raise ValueError("'rot_mat' must be provided for 'output_rot = True'")
    if rot_mat is not None:
        if ((x.shape[0] != rot_mat.shape[0])
                or (x.shape[1] != rot_mat.shape[1])):
            raise ValueError("Inconsistent shapes / number of dimensions of "
                             + "input arrays")
        if rot_mat.dtype != "float32":
            raise ValueError("'rot mat' has incorrect data type")
        rot_mat = np.ascontiguousarray(rot_mat)
    x = np.ascontiguousarray(x)
    y = np.ascontiguousarray(y)
    z = np.ascontiguousarray(z)
    vec_tilt = np.empty(x.shape + (3,), dtype=np.float32)
    L = _lib.lib()
    fn = L.hz_slope_plane_meth if which == 0 else L.hz_slope_vector_meth
    _lib.check(fn(ptr(x), ptr(y), ptr(z), x.shape[0], x.shape[1], ptr(rot_mat), int(bool(output_rot)),
                  ptr(vec_tilt), device))
    return vec_tilt


def slope_plane_meth(x, y, z, rot_mat=None, output_rot=False, *, device=0):
    """Plane-based slope computation (surface normal of the least-squares plane through the
    centre and its 8 neighbours).  Arguments and result as the reference
    (topo_param.pyx:16-82): x, y, z float32 (y, x); optional rot_mat float32 (y, x, 3, 3);
    returns vec_tilt float32 (y, x, 3) with NaN on the outermost ring."""
    return _slope(0, x, y, z, rot_mat, output_rot, device)


def slope_vector_meth(x, y, z, rot_mat=None, output_rot=False, *, device=0):
    """Vector-based slope computation (average normal of the 4 adjacent triangles,
    Corripio 2003).  Arguments and result as the reference (topo_param.pyx:230-281)."""
    return _slope(1, x, y, z, rot_mat, output_rot, device)
