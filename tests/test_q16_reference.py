"""The 16-bit horizon code (tests/q16_reference.py, DESIGN.md section 4 clause 15) pinned on the CPU: round trip, order,
error bound, clamps -- and the condition of the GPU look-up test, from the reference alone."""
import numpy as np
import pytest

from horayzon_amd import horizon
from tests import horisun_reference as R
from tests import q16_reference as Q

F = np.float32


def test_constants_agree_with_the_package():
    assert horizon.Q16_NAN == Q.NAN_CODE == 0xFFFF
    assert horizon.Q16_STEP == Q.STEP and horizon.Q16_MAX_ERROR == Q.MAX_ERROR
    assert abs(Q.MAX_ERROR - 2.4029e-5) < 1e-9
    assert abs(np.rad2deg(Q.STEP) - 0.0027) < 1e-4


def test_round_trip_of_all_codes():
    q = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = Q.decode(q)
    assert v.dtype == np.float32 and np.array_equal(Q.encode(v), q)
    assert np.isnan(v[0xFFFF]) and v.view(np.uint32)[0xFFFF] == 0x7FC00000 and not np.isnan(v[:0xFFFF]).any()
    assert v[32767] == 0.0 and not np.signbit(v[32767])
    assert v[0] == F(-Q.HALF_PI) and v[65534] == F(Q.HALF_PI)


def test_decode_is_strictly_increasing():
    v = Q.decode(np.arange(65535, dtype=np.uint32).astype(np.uint16))
    assert (np.diff(v.astype(np.float64)) > 0.0).all()


def test_error_bound_on_a_sample_and_next_to_every_boundary():
    rng = np.random.default_rng(15)
    v = rng.uniform(-Q.HALF_PI, Q.HALF_PI, 2_000_000).astype(F)
    v = v[np.abs(v.astype(np.float64)) <= Q.HALF_PI]
    err = np.abs(Q.decode(Q.encode(v)).astype(np.float64) - v.astype(np.float64))
    print("largest error of the sample: %.6g rad (bound %.6g)" % (err.max(), Q.MAX_ERROR))
    assert err.max() <= Q.MAX_ERROR
    # every float32 next to a boundary between two codes: the float32 nearest to (k + 0.5) * STEP and its two neighbours
    k = np.arange(-32767, 32767, dtype=np.float64)
    mid = ((k + 0.5) * Q.STEP).astype(F)
    near = np.concatenate([np.nextafter(mid, F(-np.inf)), mid, np.nextafter(mid, F(np.inf))])
    q = Q.encode(near)
    err = np.abs(Q.decode(q).astype(np.float64) - near.astype(np.float64))
    assert err.max() <= Q.MAX_ERROR
    assert err.max() > Q.STEP / 2 - 2.0 ** -23               # the boundaries are where the bound is approached
    lower = (k + 32767.0).astype(np.uint16)
    for part in np.split(q, 3):                              # each neighbour lands in one of the two codes of its boundary
        assert ((part == lower) | (part == lower + 1)).all()


def test_clamps_and_zeros():
    v = np.array([np.inf, -np.inf, 2.0, -2.0, 0.0, -0.0, np.nan, Q.HALF_PI, -Q.HALF_PI, 3.0e38, -3.0e38], F)
    want = [65534, 0, 65534, 0, 32767, 32767, 0xFFFF, 65534, 0, 65534, 0]
    assert Q.encode(v).tolist() == want
    back = Q.decode(Q.encode(np.array([0.0, -0.0], F)))
    assert back.view(np.uint32).tolist() == [0, 0]           # +0.0f exactly
    # NaNs of every payload and sign
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(F)
    assert (Q.encode(nans) == 0xFFFF).all()


def test_case_sprinkles_nan_and_leaves_the_rest():
    c, base = Q.case("inner_A7_random"), R.case("inner_A7_random")
    nan = np.isnan(c["hori"])
    assert 0.005 < nan.mean() < 0.05 and np.array_equal(c["hori"][~nan], base["hori"][~nan])
    assert np.array_equal(Q.case("inner_A7_random")["hori"], c["hori"], equal_nan=True)
    for k in ("suns", "mask", "vec_tilt", "vert"):
        assert np.array_equal(c[k], base[k])


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_gpu_look_up_cases_respect_the_exclusion_cap(name):
    """The condition of tests/test_gpu_q16.py::test_look_up_matches_the_reference: on decode(encode(hori)) at most CAP of
    the unmasked pairs lie within MARGIN of the terrain decision."""
    c = Q.case(name)
    c["hori"] = Q.decode(Q.encode(c["hori"]))
    ref = R.reference(c)
    share = R.inside_margin_share(c, ref)
    print("%s: share inside the margin %.3g, smallest margin %.3g rad" % (name, share, float(ref["margin"].min())))
    assert share <= R.CAP
    assert (ref["code"][:, c["mask"] != 1] == 3).all()
