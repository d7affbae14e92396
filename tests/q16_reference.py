"""DESIGN.md section 4, clause 15 in NumPy: the 16-bit horizon code.

All arithmetic is float64, every operation is rounded on its own (NumPy rounds each elementwise operation separately) and
np.rint rounds half to even.  `case(name)` is the case of tests/horisun_reference.py with NaN sprinkled over the horizon."""
import numpy as np

from tests import horisun_reference as R

HALF_PI = 1.5707963267948966
SCALE = 32767.0 / HALF_PI
STEP = HALF_PI / 32767.0
NAN_CODE = 0xFFFF
MAX_ERROR = STEP / 2 + 2.0 ** -24            # half a step plus half a float32 ulp below 2 rad


def encode(v):
    """float32 -> uint16: NaN -> 0xFFFF, else rint(clamp(v) * SCALE) + 32767 (0 ... 65534)."""
    v = np.asarray(v)
    assert v.dtype == np.float32
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(v.astype(np.float64), -HALF_PI), HALF_PI)
        q = np.rint(c * SCALE) + 32767.0
    return np.where(nan, np.float64(NAN_CODE), q).astype(np.uint16)


def decode(q):
    """uint16 -> float32: 0xFFFF -> the quiet NaN 0x7FC00000, else (float)((q - 32767) * STEP)."""
    q = np.asarray(q)
    assert q.dtype == np.uint16
    out = ((q.astype(np.int64) - 32767).astype(np.float64) * STEP).astype(np.float32)
    out.view(np.uint32)[q == NAN_CODE] = 0x7FC00000
    return out


def case(name):
    c = R.case(name)
    hori = c["hori"].copy()
    hori[np.random.default_rng(5).random(hori.shape) < 0.02] = np.nan
    c["hori"] = hori
    return c
