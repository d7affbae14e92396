"""Cases and yardstick of HorizonTerrain.sw_dir_cor_coarse (clause 12), shared by
tests/test_horisun_coarse_reference.py (CPU) and tests/test_gpu_horisun_coarse.py.

The cases are tests.horisun_reference.make_case with a few blocks masked out before anything else uses the mask, so that the
coarse grids below have empty, partly masked and full blocks.  The yardstick is the block-mean fold of per-position maps: a
float64 accumulator per coarse cell that takes the block's unmasked cells one at a time in row-major order (not np.sum),
divided by their number in float64 and rounded to float32 once."""
import numpy as np

from tests import horisun_reference as R


def _mask_big(mask):
    mask[8:12, 20:24] = 0
    mask[12:18, 20:40] = 0


def _mask_small(mask):
    mask[0:2, 0:3] = 0


# name: (make_case arguments, keyword arguments, mask edits)
_SPEC = {
    "A360": (((48, 60), (56, 68), (4, 4), 360, 7, "random", 301), {}, _mask_big),
    "A7": (((48, 60), (56, 68), (4, 4), 7, 7, "planar", 302), {"fill": -9.0}, _mask_big),
    "A2": (((48, 60), (50, 64), (2, 3), 2, 6, "random", 304), {}, _mask_big),
    "A1": (((8, 12), (8, 12), (0, 0), 1, 1, "planar", 303), {}, _mask_small),
}
NAMES = tuple(_SPEC)
PIXELS_BIG = (4, (6, 20), (48, 1), (1, 60), (48, 60), 1, (3, 5))
PIXELS = {"A360": PIXELS_BIG, "A7": PIXELS_BIG, "A2": PIXELS_BIG, "A1": ((2, 3), (8, 12), 1, (4, 1))}

_CASES = {}


def case(name):
    """(case, reference) of a name: built once per session; the arrays are read-only afterwards."""
    if name not in _CASES:
        args, kw, edit = _SPEC[name]
        c = R.make_case(*args, **kw)
        edit(c["mask"])
        ref = R.reference(c)
        for a in list(c.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[name] = (c, ref)
    return _CASES[name]


def pair(P):
    return (P, P) if isinstance(P, int) else tuple(P)


def block_counts(mask, P):
    P0, P1 = pair(P)
    gy, gx = mask.shape[0] // P0, mask.shape[1] // P1
    return (mask == 1).reshape(gy, P0, gx, P1).sum(axis=(1, 3))


def block_any(flags, P):
    """flags bool[S][y][x] -> bool[S][gy][gx]: some cell of the block is flagged."""
    P0, P1 = pair(P)
    S, y, x = flags.shape
    return flags.reshape(S, y // P0, P0, x // P1, P1).any(axis=(2, 4))


def block_means(sw, sh, mask, P, fill):
    """The contract from per-position maps sw f32[S][y][x] and sh u8[S][y][x]: (f_cor, sunlit_frac) f32[S][gy][gx].
    (block_means of tests/test_gpu_coarse.py, restated: that module is marked gpu as a whole.)"""
    P0, P1 = pair(P)
    S = sw.shape[0]
    n = block_counts(mask, P)
    acc = np.zeros((S,) + n.shape, np.float64)
    for di in range(P0):
        for dj in range(P1):
            on = np.broadcast_to(mask[di::P0, dj::P1] == 1, acc.shape)
            np.add(acc, sw[:, di::P0, dj::P1].astype(np.float64), out=acc, where=on)     # masked cells: no add at all
    lit = ((sh == 0) & (mask == 1)).reshape(S, n.shape[0], P0, n.shape[1], P1).sum(axis=(2, 4))
    some = np.broadcast_to(n > 0, acc.shape)
    nn = np.maximum(n, 1).astype(np.float64)
    f_cor = (acc / nn).astype(np.float32)
    frac = (lit.astype(np.float64) / nn).astype(np.float32)
    f_cor[~some] = fill
    frac[~some] = fill
    return f_cor, frac


def same(a, b):
    """Bit for bit; NaNs (the fill value) only have to be NaNs on both sides."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def is_fill(a, fill):
    return bool(np.isnan(a).all() if np.isnan(fill) else (a == np.float32(fill)).all())
