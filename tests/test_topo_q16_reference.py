"""The quantisation bound of the reductions on 16-bit codes (DESIGN.md section 4 clause 17), checked on the yardstick alone:
tests/topo_reference.py's `exact` column on a horizon h and on Q.decode(Q.encode(h)).  No GPU, no kernel.

With D = STEP / 2 + 2^-24 >= |decode(encode(h)) - h| for h in range: max(h, plane horizon) is 1-Lipschitz in h, the term of
the VSF, 1 - cos(pi/2 - he), and of the openness, pi/2 - h, have |d/dhe| <= 1, and the SVF's term
dot * ((pi/2 - he) - sin(2 he) / 2) + tz * cos(he)^2 has d/dhe = -dot * (1 + cos 2he) - tz * sin 2he, at most
2 |dot| + |tz| <= 2 hypot(tx, ty) + |tz| = L.  Summed over A azimuths and scaled by azim_spac / (2 pi):

    |svf(q) - svf(h)| <= L * D * A * azim_spac / (2 pi)        |vsf(q) - vsf(h)| <= D * A * azim_spac / (2 pi)
    |openness(q) - openness(h)| <= D                           (divided by A; no azimuth spacing in it)

Every ratio to the bound is printed before it is asserted <= 1 (pytest -s)."""
import numpy as np
import pytest

from tests import q16_reference as Q
from tests import topo_reference as R

D = Q.STEP / 2 + 2.0 ** -24

# (label, cells, azimuths, start of the azimuths, tilt, share of entries at +-float32(pi/2))
CASES = [
    ("A=2 slopes<=70", (5, 41), 2, 0.0, lambda rng, s: R.tilt_slopes(rng, s, 70.0), 0.05),
    ("A=33 slopes<=89.5", (5, 205), 33, 0.37, lambda rng, s: R.tilt_slopes(rng, s, 89.5), 0.05),
    ("A=90 unnormalised", (5, 205), 90, 0.37, lambda rng, s: R.tilt_slopes(rng, s, 70.0, length=(0.5, 3.0)), 0.05),
    ("A=360 up and slopes<=35", (4, 100), 360, 0.0,
     lambda rng, s: np.concatenate([R.tilt_up((2, s[1])), R.tilt_slopes(rng, (2, s[1]), 35.0)]), 0.05),
]


def test_the_constant():
    assert D == Q.MAX_ERROR and 2.40e-5 < D < 2.41e-5


@pytest.mark.parametrize("label,shape,A,start,make_tilt,frac", CASES, ids=[c[0] for c in CASES])
def test_quantisation_bound_on_the_exact_reference(label, shape, A, start, make_tilt, frac):
    rng = np.random.default_rng(1000 + A)
    azim = R.make_azim(A, start=start)
    tilt = make_tilt(rng, shape)
    h = R.hori_uniform(rng, shape, A, frac_half_pi=frac)
    assert (np.abs(h) == np.float32(np.pi / 2)).mean() > frac / 2
    hq = Q.decode(Q.encode(h))
    assert float(np.abs(hq.astype(np.float64) - h.astype(np.float64)).max()) <= D
    a, b = R.topo_reference(azim, h, tilt), R.topo_reference(azim, hq, tilt)
    sector = A * (float(azim[1]) - float(azim[0])) / (2.0 * np.pi)
    t = tilt.astype(np.float64)
    bound = {"svf": (2.0 * np.hypot(t[..., 0], t[..., 1]) + np.abs(t[..., 2])) * D * sector,
             "vsf": np.full(shape, D * sector), "openness": np.full(shape, D)}
    worst = {}
    for name in R.NAMES:
        diff = np.abs(b[name].exact - a[name].exact)
        assert np.isfinite(diff).all()
        worst[name] = float((diff / bound[name]).max())
        print("TOPOQ16REF %-26s %-8s max |exact(q) - exact(h)| %.3g  worst ratio to the bound %.3f"
              % (label, name, float(diff.max()), worst[name]))
    for name in R.NAMES:
        assert worst[name] <= 1.0, (label, name, worst[name])
