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


def _contiguous_planes(hori):
    # (np.ascontiguousarray of the cell-major path would silently copy 18 GB of planes)
    if not hori.flags["C_CONTIGUOUS"]:
        raise ValueError("array 'hori' is not C-contiguous")
    return hori


TOPO_NAMES = ("svf", "vsf", "openness")
# a single output on a cell-major horizon keeps its own entry point (the exports stay exercised)
_SINGLE = {"svf": "hz_sky_view_factor", "vsf": "hz_visible_sky_fraction", "openness": "hz_topographic_openness"}


def _reduce(names, azim, hori, vec_tilt, device, layout, single=False):
    """``{name: float32 (y, x)}`` for the ``names`` out of TOPO_NAMES: the reference's shape and dtype checks
    (topo_param.pyx:398-404, :486-492, :565-569), the contiguity handling and the library call.  ``single``: ``names`` is
    one name, and a cell-major horizon goes to that output's own entry point."""
    tilted = "svf" in names or "vsf" in names
    planes, cells, num = _cell_shape(hori, layout)
    if tilted:
        if (len(azim) != num) or (cells != vec_tilt.shape[:2])\
                or (vec_tilt.shape[2] != 3):
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
        if ((azim.dtype != "float32") or (hori.dtype != "float32")
                or (vec_tilt.dtype != "float32")):
            raise ValueError("Input array(s) has/have incorrect data type(s)")
        if len(azim) < 2:   # azim[1] - azim[0] is read (topo_param.pyx:433, :520): out of bounds in the reference
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
        vec_tilt = np.ascontiguousarray(vec_tilt)
    else:
        if len(azim) != num:
            raise ValueError("Inconsistent/incorrect shapes of input arrays")
        if (azim.dtype != "float32") or (hori.dtype != "float32"):
            raise ValueError("Input array(s) has/have incorrect data type(s)")
        vec_tilt = None
    azim = np.ascontiguousarray(azim)
    hori = _contiguous_planes(hori) if planes else np.ascontiguousarray(hori)
    out = {n: np.empty(cells, dtype=np.float32) for n in TOPO_NAMES if n in names}
    L = _lib.lib()
    if single and not planes:
        tilt_arg = (ptr(vec_tilt),) if tilted else ()
        _lib.check(getattr(L, _SINGLE[names[0]])(ptr(azim), ptr(hori), *tilt_arg, cells[0], cells[1], num,
                                                 ptr(out[names[0]]), device))
    else:
        _lib.check((L.hz_topo_params_planes if planes else L.hz_topo_params)(
            ptr(azim), ptr(hori), ptr(vec_tilt), cells[0], cells[1], num, ptr(out.get("svf")), ptr(out.get("vsf")),
            ptr(out.get("openness")), device))
    return out


def sky_view_factor(azim, hori, vec_tilt, *, device=0, layout="cell_major"):
    """Sky view factor (SVF) computation.

    Same arguments, checks and result as the reference
    (topo_param.pyx:377-409): azim float32 (azim), hori float32 (y, x, azim)
    [radian], vec_tilt float32 (y, x, 3); returns svf float32 (y, x).  With
    ``layout="azim_major"`` (not in the reference) hori is float32 (azim, y, x), C-contiguous; the result is the
    same, bit for bit."""
    return _reduce(["svf"], azim, hori, vec_tilt, device, layout, single=True)["svf"]


def visible_sky_fraction(azim, hori, vec_tilt, *, device=0, layout="cell_major"):
    """Visible sky fraction (solid angle of the visible sky); arguments, checks and result as the
    reference (topo_param.pyx:465-496); ``layout`` as in ``sky_view_factor``."""
    return _reduce(["vsf"], azim, hori, vec_tilt, device, layout, single=True)["vsf"]


def topographic_openness(azim, hori, *, device=0, layout="cell_major"):
    """Positive topographic openness (Yokoyama et al. 2002) [radian]; arguments, checks and result as
    the reference (topo_param.pyx:548-574); ``layout`` as in ``sky_view_factor``."""
    return _reduce(["openness"], azim, hori, None, device, layout, single=True)["openness"]


def topo_parameters(azim, hori, vec_tilt=None, which=TOPO_NAMES, *, device=0, layout="cell_major"):
    """Any of the three reductions above -- sky view factor ("svf"), visible sky fraction ("vsf"),
    positive topographic openness ("openness") -- from ONE pass over the horizon array
    (hz_topo_params).  Arguments and checks as the single-output functions (topo_param.pyx:398-404,
    :486-492, :565-569); ``vec_tilt`` is needed for "svf" and "vsf" only.  Returns
    ``{name: float32 (y, x)}``, each map bit-identical to the single-output function's.  ``layout="azim_major"``: hori is
    float32 (azim, y, x), C-contiguous (hz_topo_params_planes); the maps are the same, bit for bit."""
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
