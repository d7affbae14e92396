"""The cases of tests/test_gpu_horisun_coarse.py, from the NumPy reference alone (no GPU): no (cell, position) pair of any case
lies inside the margin of the terrain decision, so every block of every coarse grid is held to the reference bit for bit, and
the masks give the coarse grids empty, partly masked and full blocks."""
import numpy as np
import pytest

from tests import horisun_coarse_cases as K
from tests import horisun_reference as R

# the smallest margin |alpha - h| of each case [rad], as computed here (the assertion below is the share inside R.MARGIN)
SMALLEST = {"A360": 2.3e-4, "A7": 1.2e-5, "A2": 6.8e-5, "A1": 1.0e-2}


@pytest.mark.parametrize("name", K.NAMES)
def test_no_block_holds_a_pair_inside_the_margin(name):
    c, ref = K.case(name)
    share = R.inside_margin_share(c, ref)
    smallest = float(ref["margin"].min())
    print("%s: share inside the margin %.3g, smallest margin %.3g rad" % (name, share, smallest))
    assert share <= R.CAP
    assert share == 0.0
    assert 0.5 * SMALLEST[name] < smallest < 2.0 * SMALLEST[name]
    inside = ref["margin"] <= R.MARGIN
    for P in K.PIXELS[name]:
        assert not K.block_any(inside, P).any(), P


@pytest.mark.parametrize("name", K.NAMES)
def test_masks_and_sunlit_fractions(name):
    c, ref = K.case(name)
    mask, fill = c["mask"], c["fill"]
    if name != "A1":
        n = K.block_counts(mask, 4)
        empty, partly, full = int((n == 0).sum()), int(((n > 0) & (n < 16)).sum()), int((n == 16).sum())
        assert empty >= 1 and partly >= 5 and full >= 1
        assert n.size == 180
        if name == "A360":
            assert (empty, partly, full) == (6, 165, 9)
        for P in ((6, 20), (3, 5)):
            assert (K.block_counts(mask, P) == 0).any(), P
    else:
        assert (K.block_counts(mask, (2, 3)) == 0).any()
    for P in K.PIXELS[name]:
        f_cor, frac = K.block_means(ref["val"], ref["code"], mask, P, fill)
        n = np.broadcast_to(K.block_counts(mask, P), frac.shape)
        assert K.is_fill(f_cor[n == 0], fill) and K.is_fill(frac[n == 0], fill), P
        if K.pair(P) != (1, 1):
            assert ((frac[n > 0] > 0) & (frac[n > 0] < 1)).any(), P
        else:
            assert set(np.unique(frac[n > 0])) <= {0.0, 1.0}
