"""The NumPy reference of HorizonTerrain.sun_times (tests/suntimes_reference.py; DESIGN.md section 4, clause 14) against
hand-made cases with analytic answers, against the shadow codes of the clause 10 / 13 references, and the properties of the
GPU cases that make tests/test_gpu_suntimes.py mean something: the exclusion cap, event times away from the sample times,
and a refraction case the switch really changes.  No GPU."""
import numpy as np
import pytest

from tests import horisun_reference as R
from tests import horisun_refrac_reference as RR
from tests import suntimes_reference as T

F = np.float32


def hand_case(hori_row, tilt=(0.0, 0.0, 1.0)):
    """One cell at the origin in the planar frame (east = x, north = y, up = z) under the horizon row `hori_row`."""
    A = len(hori_row)
    tilt = np.asarray(tilt, np.float64)
    tilt = tilt / np.linalg.norm(tilt)
    return dict(azim_num=A, hori=np.asarray(hori_row, F).reshape(1, 1, A), vert=np.zeros((1, 1, 3), F),
                vec_tilt=tilt.astype(F).reshape(1, 1, 3), vec_norm=np.array([0, 0, 1], F).reshape(1, 1, 3),
                vec_north=np.array([0, 1, 0], F).reshape(1, 1, 3), surf_enl_fac=np.ones((1, 1), F),
                mask=np.ones((1, 1), np.uint8), fill=np.nan, ang_max=89.0)


def suns_at(az_deg, el_rad):
    az, el = np.deg2rad(np.asarray(az_deg, np.float64)), np.asarray(el_rad, np.float64)
    d = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], axis=1)
    return (1.5e11 * d).astype(F)


# a sun 1.5e11 m away stored in float32 is placed to 2^14 m: 1e-7 rad, which at the rates below is 1e-6 of a time unit
HAND_TOL = 1.0e-5


def one(ref, key):
    return float(ref[key][0, 0])


def test_linear_clearance_gives_the_closed_form_crossing():
    """Constant horizon 0.2 rad, flat surface, the sun climbing 0.1 rad per hour at one azimuth: g = elevation - 0.2 is
    linear, the crossing is where the elevation is 0.2 rad."""
    c = hand_case([0.2] * 12)
    times = np.arange(6, dtype=np.float64)
    ref = T.sun_times(c, suns_at([135.0] * 6, 0.02 + 0.1 * times), times)
    assert one(ref, "intervals") == 1
    assert abs(one(ref, "sunrise") - 1.8) <= HAND_TOL
    assert one(ref, "sunset") == 5.0                              # lit at the end: the last time
    assert abs(one(ref, "duration") - 3.2) <= HAND_TOL
    # non-uniform times: the crossing is 0.8 of the way from times[1] to times[2]
    uneven = np.array([0.0, 0.5, 3.0, 3.25, 4.0, 9.0])
    ref = T.sun_times(c, suns_at([135.0] * 6, 0.02 + 0.1 * times), uneven)
    assert abs(one(ref, "sunrise") - 2.5) <= HAND_TOL and one(ref, "sunset") == 9.0
    assert abs(one(ref, "duration") - 6.5) <= HAND_TOL


def test_lit_at_both_ends_gives_the_first_and_last_time():
    c = hand_case([-0.5] * 7)
    times = np.array([3.0, 4.5, 5.0, 8.0])
    ref = T.sun_times(c, suns_at([100.0, 150.0, 200.0, 250.0], [0.2, 0.5, 0.5, 0.2]), times)
    assert one(ref, "sunrise") == 3.0 and one(ref, "sunset") == 8.0
    assert one(ref, "duration") == 5.0 and one(ref, "intervals") == 1
    assert ref["lit"].all()


def test_a_peak_that_interrupts_the_sun_gives_two_spells():
    """36 azimuths: horizon 0.1 rad with a peak of 0.6 rad at 170 - 190 degrees; the sun at 0.3 rad goes from 120 to 240
    degrees in steps of 10: h is linear in s between the nodes, it passes 0.3 rad at 164 and at 196 degrees."""
    row = np.full(36, 0.1)
    row[17:20] = 0.6
    c = hand_case(row)
    times = np.arange(13, dtype=np.float64)
    ref = T.sun_times(c, suns_at(120.0 + 10.0 * times, [0.3] * 13), times)
    assert one(ref, "intervals") == 2
    assert one(ref, "sunrise") == 0.0 and one(ref, "sunset") == 12.0
    assert abs(one(ref, "duration") - (4.4 + (12.0 - 7.6))) <= HAND_TOL
    assert list(ref["lit"][:, 0, 0]) == [True] * 5 + [False] * 3 + [True] * 5


def test_a_curved_clearance_is_bracketed_by_its_samples():
    """A surface tilted 40 degrees towards the west under a horizon far below: the surface decides (g = asin(dot_ts), not
    linear in time).  The interpolated sunrise lies strictly between the two samples that bracket it, and within the chord
    error of a track 100 times finer."""
    c = hand_case([-0.5] * 12, tilt=(-np.sin(np.deg2rad(40.0)), 0.0, np.cos(np.deg2rad(40.0))))
    x = np.linspace(0.0, 1.0, 13)
    coarse = T.sun_times(c, suns_at(90.0 + 180.0 * x, np.deg2rad(5.0 + 50.0 * np.sin(np.pi * x))), 12.0 * x)
    xf = np.linspace(0.0, 1.0, 1201)
    fine = T.sun_times(c, suns_at(90.0 + 180.0 * xf, np.deg2rad(5.0 + 50.0 * np.sin(np.pi * xf))), 12.0 * xf)
    lit = coarse["lit"][:, 0, 0]
    first = int(np.argmax(lit))
    assert 0 < first and not lit[:first].any()
    assert 12.0 * x[first - 1] < one(coarse, "sunrise") < 12.0 * x[first]
    assert one(coarse, "intervals") == one(fine, "intervals") == 1
    assert abs(one(coarse, "sunrise") - one(fine, "sunrise")) < 0.1          # a tenth of the step of 1.0
    assert one(coarse, "sunset") == one(fine, "sunset") == 12.0


def test_never_lit_and_masked_cells():
    c = hand_case([1.2] * 5)
    times = np.arange(4, dtype=np.float64)
    ref = T.sun_times(c, suns_at([90.0, 120.0, 150.0, 180.0], [0.1, 0.4, 0.4, 0.1]), times)
    assert np.isnan(one(ref, "sunrise")) and np.isnan(one(ref, "sunset"))
    assert one(ref, "duration") == 0.0 and one(ref, "intervals") == 0
    c["mask"][:] = 0
    c["fill"] = -1.0
    ref = T.sun_times(c, suns_at([90.0, 120.0, 150.0, 180.0], [0.1, 0.4, 0.4, 0.1]), times)
    assert one(ref, "sunrise") == one(ref, "sunset") == one(ref, "duration") == -1.0 and one(ref, "intervals") == -1


@pytest.mark.parametrize("name", T.NAMES)
def test_lit_is_shadow_code_zero(name):
    c, refs = T.case(name)
    args = (c["suns"], c["hori"], c["vert"], c["vec_tilt"], c["vec_norm"], c["vec_north"], c["surf_enl_fac"], c["mask"],
            c["fill"], c["ang_max"])
    codes = (R.lookup(*args) if c["fac"] is None else RR.lookup_refrac(*args, c["fac"]))["code"]
    unmasked = c["mask"] == 1
    for fl in T.FLAVOURS:
        ref = refs[fl]
        assert np.array_equal(ref["lit"][:, unmasked], codes[:, unmasked] == 0)
        assert np.array_equal(ref["intervals"][unmasked], T.runs_of_zero(codes)[unmasked])
        assert (ref["intervals"][~unmasked] == -1).all()


@pytest.mark.parametrize("flavour", T.FLAVOURS)
@pytest.mark.parametrize("name", T.NAMES)
def test_the_reference_alone_stays_under_the_exclusion_cap(name, flavour):
    c, refs = T.case(name)
    share = T.excluded_share(c, refs[flavour])
    print("%s %s: %.4f of the unmasked cells excluded" % (name, flavour, share))
    assert share <= T.CAP
    t = c["times"][flavour]
    assert np.isfinite(t).all() and (np.diff(t) > 0.0).all()
    if len(t) > 1:
        assert 0.25 <= np.diff(t).min() and np.diff(t).max() <= 2.0


def test_the_cases_reach_what_they_are_for():
    _, refs = T.case("inner_A360_planar")
    assert T.case("inner_A360_planar")[0]["mask"].size % 256 != 0
    assert refs["uniform"]["intervals"].max() >= 3                # several spells
    c, refs = T.case("inner_A1_random")
    never = (refs["uniform"]["intervals"] == 0) & (c["mask"] == 1)
    assert never.any()                                            # NaN, NaN, 0.0, 0 on the GPU too
    assert np.isnan(refs["uniform"]["sunrise"][never]).all() and (refs["uniform"]["duration"][never] == 0.0).all()
    c, refs = T.case("one_position")
    assert c["suns"].shape[0] == 1 and (refs["uniform"]["intervals"] == 1).any()
    lit = refs["uniform"]["intervals"] == 1
    assert (refs["uniform"]["sunrise"][lit] == F(c["times"]["uniform"][0])).all()
    assert (refs["uniform"]["duration"][lit] == 0.0).all()
    c, refs = T.case("all_masked")
    assert (refs["uneven"]["intervals"] == -1).all() and np.isnan(refs["uneven"]["duration"]).all()
    c, refs = T.case("fill_minus_one")
    assert (refs["uneven"]["sunset"][c["mask"] != 1] == -1.0).all() and (c["mask"] != 1).any()


@pytest.mark.parametrize("flavour", T.FLAVOURS)
@pytest.mark.parametrize("name", T.MULTI_CELL + (T.REFRAC,))
def test_event_times_are_not_sample_times(name, flavour):
    """More than half of the scored cells have a sunrise more than 100 tolerances from the nearest sample time: a kernel that
    returns sample times fails the GPU comparison."""
    c, refs = T.case(name)
    ref, times = refs[flavour], c["times"][flavour]
    sc = T.scored(c, ref)
    tol = T.tolerances(ref, times)[0]
    with np.errstate(all="ignore"):
        off = np.abs(ref["sunrise"].astype(np.float64)[..., None] - times).min(axis=-1)
        away = sc & (ref["intervals"] > 0) & (off > 100.0 * tol)
    print("%s %s: %d of %d scored cells" % (name, flavour, int(away.sum()), int(sc.sum())))
    assert away.sum() > 0.5 * sc.sum()


@pytest.mark.parametrize("flavour", T.FLAVOURS)
def test_refraction_moves_the_sunrise_of_the_refraction_case(flavour):
    c, refs = T.case(T.REFRAC)
    ref, plain = refs[flavour], T.case_plain_reference(T.REFRAC, flavour)
    unmasked = c["mask"] == 1
    tol = T.tolerances(ref, c["times"][flavour])[0]
    with np.errstate(all="ignore"):
        moved = np.abs(ref["sunrise"].astype(np.float64) - plain["sunrise"].astype(np.float64)) > tol
    moved |= np.isnan(ref["sunrise"]) != np.isnan(plain["sunrise"])
    share = float((moved & unmasked).sum()) / unmasked.sum()
    print("refraction moves the sunrise of %.3f of the cells" % share)
    assert share > 0.01
