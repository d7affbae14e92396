"""Argument validation of the drop-in boundary as data.

The reference checks its arguments in a fixed order and raises fixed exception classes with fixed messages
(horizon.pyx:108-153, :279-312; shadow.pyx:87-133); callers and tests depend on class, message and ORDER, so those are the
contract.  Here every entry point states its checks as a table of rules -- (exception class, message, predicate that is true
when the argument is BAD) -- and `run` raises the first rule that fires.  Predicates are callables so that a later rule may
rely on what an earlier one established (shapes before contents).

What Terrain's observer and ray calls (viewshed, sight_height, panorama, cast) have in common is stated here once: `is_number`
and `all_finite` for their predicates, and the makers of the three rules every one of them has -- `some_output_given`,
`all_contiguous`, `distinct_outputs` -- which a call lists in its table like any other rule, at its place in the order."""
import numpy as np

from ._lib import ptr

ALGORITHMS = ("discrete_sampling", "binary_search", "guess_constant")
GEOMETRIES = ("triangle", "quad", "grid")
DIM_LIMIT = 32767          # Embree's 16-bit grid resolution, kept as the reference's limit (horizon.pyx:149-151)

MSG_ALG = "invalid input argument for ray_algorithm"
MSG_GEOM = "invalid input argument for geom_type"
MSG_ACC = "limit of hori_acc (10 degree) is exceeded"
MSG_ELEV = "minimal allowed value for 'ray_org_elev' is 0.005 m"
MSG_MASK_TYPE = "data type of mask must be 'uint8'"
MSG_DIM_LIMIT = "maximal allowed input length for dem_dim_0 and dem_dim_1 is 32'767"
MSG_NORTH = "dimension (lengths) of vec_norm and/or vec_north is/are erroneous"


def run(rules):
    """rules: iterable of (exception class, message, is_bad) -- raises the first whose predicate returns true."""
    for exc, message, is_bad in rules:
        if is_bad():
            raise exc(message)


def same_leading_shape(arrays, ndim, n_lead):
    """True when every array has `ndim` dimensions and they agree with the first one in their leading `n_lead` lengths."""
    first = arrays[0]
    return all(a.ndim == ndim for a in arrays) and all(a.shape[:n_lead] == first.shape[:n_lead] for a in arrays)


def fits_grid(n_elements, dem_dim_0, dem_dim_1):
    return n_elements >= dem_dim_0 * dem_dim_1 * 3


def window_inside(offset_0, offset_1, shape, dem_dim_0, dem_dim_1):
    return offset_0 + shape[0] <= dem_dim_0 and offset_1 + shape[1] <= dem_dim_1


def unit_vectors(v, tol=1.0e-5):
    return float(np.abs((v ** 2).sum(axis=2) - 1.0).max()) <= tol


def is_number(v):
    """An int, a float or a NumPy scalar of either kind; a bool is not a number."""
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def all_finite(a):
    """Whether a NumPy array or a torch tensor has finite entries only (a tensor: a reduction on its device, read back)."""
    if isinstance(a, np.ndarray):
        return bool(np.isfinite(a).all())
    import torch
    return bool(torch.isfinite(a).all().item())


def contiguous(a):
    return a.flags["C_CONTIGUOUS"] if isinstance(a, np.ndarray) else a.is_contiguous()


def quoted_names(outs):
    """'a', 'b' and 'c' of an outputs table (("a", ...), ("b", ...), ("c", ...))."""
    names = ["'%s'" % row[0] for row in outs]
    return ", ".join(names[:-1]) + " and " + names[-1]


def some_output_given(outs, given):
    """`outs`: the call's outputs table, a row per output that starts with its name; `given`: the buffers that are not None."""
    return (ValueError, "at least one of %s must be given" % quoted_names(outs), lambda: not given)


def all_contiguous(arrays):
    """`arrays`: a callable that gives the list, since an earlier rule may have to hold before it can be formed."""
    return (ValueError, "not all input arrays are C-contiguous", lambda: not all(contiguous(a) for a in arrays()))


def distinct_outputs(outs, given):
    return (ValueError, "%s must be different arrays" % quoted_names(outs), lambda: len({ptr(buf) for buf in given}) != len(given))
