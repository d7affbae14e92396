"""The HOST build of hz_crmath.h against tests/golden/crmath_reference.npz (mpmath at 200 bits, rounded once to float32:
tests/golden/make_crmath_fixture.py).  tests/test_gpu_crmath.py holds the device build to the same file and to this build."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fixture():
    d = np.load(os.path.join(GOLDEN, "crmath_reference.npz"))
    return {k: d[k] for k in d.files}


def _generator():
    spec = importlib.util.spec_from_file_location("make_crmath_fixture", os.path.join(GOLDEN, "make_crmath_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_build_equals_the_mpmath_fixture(orc):
    """Word for word (no NaN occurs in these ranges; one would have to be a NaN on both sides).  Entries flagged is_hard -- the
    exact value within the header's 1e-14 of a rounding boundary -- are left out and number at most 2."""
    fx = _fixture()
    which, x, ref, hard = (fx[k] for k in ("which", "x", "ref", "is_hard"))
    assert x.dtype == np.float32 and ref.dtype == np.float32 and hard.dtype == np.bool_ and len(x) > 24000
    assert hard.sum() <= 2
    y = np.full(x.shape, fx["pow_y"], np.float32)
    orc.set_libm(False)
    for k, name in enumerate(orc.CRMATH_FUNCS[:5]):
        m = which == k
        assert m.sum() > 4000, name
        host = orc.crmath_eval(k, x[m], y[m])
        d = (host.view(np.uint32) != ref[m].view(np.uint32)) & ~(np.isnan(host) & np.isnan(ref[m])) & ~hard[m]
        assert not d.any(), (name, x[m][d][:5], host[d][:5], ref[m][d][:5])
    assert set(np.unique(which)) == set(range(5))


def test_fixture_is_not_the_platform_libm(orc):
    """The file can tell a correctly rounded routine from one that is not: glibc's acosf / tanf miss it on some arguments."""
    fx = _fixture()
    which, x, ref = (fx[k] for k in ("which", "x", "ref"))
    orc.set_libm(True)
    try:
        bad = {k: int((orc.crmath_eval(k, x[which == k]).view(np.uint32) != ref[which == k].view(np.uint32)).sum())
               for k in (0, 1)}
    finally:
        orc.set_libm(False)
    print("words of the platform's acosf / tanf that differ from the fixture:", bad)
    assert bad[0] > 0 and bad[1] > 0


def test_stored_arguments_are_the_recipe(orc):
    """The generator's argument recipe, re-run with the committed seed (NumPy only), gives the stored arguments bit for bit,
    and the recipe covers what it says: both sqrt branches of acos, the floats on both sides of every switch."""
    fx = _fixture()
    gen = _generator()
    assert int(fx["seed"]) == gen.SEED
    which, x = gen.arguments(int(fx["seed"]))
    assert np.array_equal(which, fx["which"]) and np.array_equal(x.view(np.uint32), fx["x"].view(np.uint32))
    assert fx["pow_y"] == gen.pow_exponent() and fx["pow_y"].dtype == np.float32
    f = {name: x[which == k] for k, name in enumerate(gen.FUNCS)}
    a = f["acos"]
    for s in (1.0, -1.0):
        assert (s * a > 0.5).sum() > 1500 and ((s * a > 0) & (s * a < 0.5)).sum() > 1500
        assert (a == np.float32(s)).any() and (a == np.float32(s * 0.5)).any()
        half = np.float32(s * 0.5)
        assert (a == np.nextafter(half, np.float32(0))).any() and (a == np.nextafter(half, np.float32(s))).any()
    assert np.abs(a).max() == 1.0 and (a == 0).sum() == 2 and np.signbit(a[a == 0]).sum() == 1
    for name, switches in (("tan", (np.pi / 4, np.pi / 2, 2.0 ** -5)), ("cos", (2.0 ** -5,)), ("sin", (2.0 ** -5,)),
                           ("pow", (1.0, 0.75))):
        for v in switches:
            c = np.float32(v)
            for k in (c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(9))):
                assert (f[name] == k).any(), (name, v)
    assert f["tan"].min() >= np.float32(0.02) and f["tan"].max() <= np.float32(1.62)
    assert f["pow"].min() >= np.float32(0.6) and f["pow"].max() <= np.float32(1.1)
