"""Generator of tests/golden/crmath_reference.npz: the correctly rounded float32 of the five functions of hz_crmath.h
(horayzon_amd/csrc), computed with mpmath at 200 bits -- a reference that shares no code, no libm and no compiler with either
build of the header.  Run from the repository root:  python tests/golden/make_crmath_fixture.py

The tests only read the .npz (tests/test_crmath_reference.py, tests/test_gpu_crmath.py); mpmath is needed here alone.
`arguments()` needs NumPy only: the CPU test re-runs it to show that the stored arguments are the recipe's.

Arguments (float32, fixed by SEED; "random" = uniform over the BIT PATTERNS between the two bounds, so every binade gets its
share; "around v" = the float nearest to v and its 8 neighbours on either side, 17 floats):
  acos  random over [0.5, 1], [-1, -0.5], [1e-20, 0.5], [-0.5, -1e-20]; around +0.5 and -0.5 (the switch to the sqrt branches);
        1, -1 and the 9 floats next to each inside [-1, 1]; +0, -0
  tan   random over [0.02, 1.62]; around pi/4 (the fold), pi/2 (the pole) and 2^-5 (the switch of sin_k / cos_k)
  cos   random over [1e-12, 0.02] and [0.02, pi/4]; around 2^-5
  sin   the same recipe, its own draws
  pow   base random over [0.6, 1.1]; around 1 and 0.75 (log's mantissa switch at 1.5 / 2); the exponent is the pressure
        formula's float32(9.81) / (float32(287) * float32(0.0065))

Rounding: v = f(x) at 200 bits; the candidate float32(float64(v)) may be double rounded, so the candidate and its two
neighbours are compared with v exactly (200-bit subtraction) and the nearest wins.

is_hard: an argument where the host (gcc) build of hz_crmath.h differs from this reference -- the exact value lies within the
header's 1e-14 of a rounding boundary, about 1 argument in 1e7.  Such an entry stays in the file, flagged; the tests compare
it device against host only.  More than MAX_HARD of them means something else is wrong: the generator stops.
"""
import os
import sys

import numpy as np

SEED = 950355
FUNCS = ("acos", "tan", "cos", "sin", "pow")       # index = `which` of hz_debug_crmath_eval / oracle.crmath_eval
MAX_HARD = 2
N_RANDOM = {"acos": 2000, "tan": 5000, "cos": 2000, "sin": 2000, "pow": 4000}      # per range
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "crmath_reference.npz")
F = np.float32


def pow_exponent():
    return F(9.81) / (F(287.0) * F(0.0065))


def _bits(v):
    return int(np.array(v, F).view(np.uint32))


def _random(rng, lo, hi, n, negative=False):
    """n floats whose bit patterns are uniform over [bits(lo), bits(hi)], 0 < lo < hi; negative: with the sign bit set."""
    u = rng.integers(_bits(lo), _bits(hi), size=n, endpoint=True, dtype=np.uint64).astype(np.uint32)
    if negative:
        u |= np.uint32(0x80000000)
    return u.view(F)


def _around(v, below=8, above=8, negative=False):
    """The float nearest to v > 0 with `below` floats under it and `above` over it (in magnitude)."""
    u = (_bits(v) + np.arange(-below, above + 1, dtype=np.int64)).astype(np.uint32)
    if negative:
        u |= np.uint32(0x80000000)
    return u.view(F)


def arguments(seed=SEED):
    """(which uint8[N], x float32[N]): the arguments of the fixture, in the file's order."""
    rng = np.random.default_rng(seed)
    pi = np.pi
    n = N_RANDOM
    parts = {
        "acos": [_random(rng, 0.5, 1.0, n["acos"]), _random(rng, 0.5, 1.0, n["acos"], negative=True),
                 _random(rng, 1e-20, 0.5, n["acos"]), _random(rng, 1e-20, 0.5, n["acos"], negative=True),
                 _around(0.5), _around(0.5, negative=True), _around(1.0, 9, 0), _around(1.0, 9, 0, negative=True),
                 np.array([0.0, -0.0], F)],
        "tan": [_random(rng, 0.02, 1.62, n["tan"]), _around(pi / 4), _around(pi / 2), _around(2.0 ** -5)],
        "cos": [_random(rng, 1e-12, 0.02, n["cos"]), _random(rng, 0.02, pi / 4, n["cos"]), _around(2.0 ** -5)],
        "sin": [_random(rng, 1e-12, 0.02, n["sin"]), _random(rng, 0.02, pi / 4, n["sin"]), _around(2.0 ** -5)],
        "pow": [_random(rng, 0.6, 1.1, n["pow"]), _around(1.0), _around(0.75)],
    }
    which = np.concatenate([np.full(sum(len(p) for p in parts[f]), k, np.uint8) for k, f in enumerate(FUNCS)])
    x = np.concatenate([p for f in FUNCS for p in parts[f]]).astype(F)
    return which, x


def _round_once(v, mp):
    """The float32 nearest to the 200-bit value v: the nearest of the candidate and its two neighbours, compared exactly."""
    c = F(float(v))
    cands = (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf)))
    dist = [abs(mp.mpf(float(k)) - v) if np.isfinite(k) else mp.inf for k in cands]
    best = min(range(3), key=lambda k: dist[k])
    assert sum(1 for d in dist if d == dist[best]) == 1, "a tie at 200 bits: %r" % (v,)
    return cands[best]


def reference(which, x):
    """float32[N]: the correctly rounded f(x) by mpmath at 200 bits."""
    import mpmath as mp
    mp.mp.prec = 200
    y = mp.mpf(float(pow_exponent()))
    fn = (mp.acos, mp.tan, mp.cos, mp.sin, lambda a: mp.power(a, y))
    out = np.empty(len(x), F)
    for i, (w, xi) in enumerate(zip(which, x)):
        out[i] = _round_once(fn[int(w)](mp.mpf(float(xi))), mp)
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import oracle
    which, x = arguments()
    ref = reference(which, x)
    host = np.empty_like(ref)
    y = np.full(len(x), pow_exponent(), F)
    oracle.set_libm(False)
    for k in range(len(FUNCS)):
        m = which == k
        host[m] = oracle.crmath_eval(k, x[m], y[m])
    is_hard = host.view(np.uint32) != ref.view(np.uint32)
    for i in np.flatnonzero(is_hard):
        print("hard: %s(%r) = %r by mpmath, %r by the host build" % (FUNCS[which[i]], x[i], ref[i], host[i]))
    if is_hard.sum() > MAX_HARD:
        raise SystemExit("%d arguments differ between mpmath and the host build (at most %d expected): not written"
                         % (is_hard.sum(), MAX_HARD))
    np.savez_compressed(PATH, seed=np.int64(SEED), which=which, x=x, ref=ref, is_hard=is_hard, pow_y=pow_exponent())
    print("%s: %d arguments (%s), %d hard, %d bytes"
          % (PATH, len(x), ", ".join("%s %d" % (f, (which == k).sum()) for k, f in enumerate(FUNCS)), is_hard.sum(),
             os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
