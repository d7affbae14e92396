"""Every instantiation of the horizon reductions -- k_topo<WANT> and k_topo_wide<WANT>, a single output being WANT = 1, 2
or 4 (horayzon_amd/csrc/hz_topo.hip) -- against the float64 NumPy reference of
tests/topo_reference.py (pinned to the real program's outputs by tests/test_topo_reference.py), not against each other.

Every case runs through the three single-output entry points, topo_parameters for all three maps and for each pair, each in
the tiled and in the one-lane-per-cell ("wide") form.  Bars:

openness      bit-identical to `contract` on every path: each operation is one IEEE float64 / float32 operation.
wide SVF/VSF  the float64 terms of `contract` with the device's sin / cos / atan for the host's.  Moving every term of
              `contract` by +-2 float64 ulps on the CPU changes the float32 result of a share `p` of the cells (measured:
              0 of 420 000 cells at 36 azimuths, 0 of 130 at 5000, up to 0.8 % only under the normal (0, 0, 1), whose
              terms are short binary fractions that land on rounding ties; the expected share is 4 ulp64 / ulp32 = 7e-9
              per addition).  At most max(10 p, 1e-4) of a case's cells may differ from `contract` (the cap next to the
              measured share in every printed line; on an MI355X no cell of any case differed), and each of those by no
              more than one float32 ulp of the accumulator, scaled to the output, plus the output's own rounding.
tiled SVF/VSF max |gpu - exact| <= E_ref + B per case: E_ref = max |contract - exact| is the reference's own error on that
              input (its float32 accumulator), computed here from the reference alone; B = 2.4e-7 is the figure the
              project publishes for its float32 terms (README.md, the kernel's header), added once because the terms
              are averaged.  Steeper than 70 degrees the float32 rounding of the plane's tangent (two terms of size ~100
              cancel) dominates E_ref and the kernel, which forms the quotients first, draws its own error of that
              size: 2 E_ref + B.  Measured on an MI355X: the kernels exceed E_ref by 1.2e-7 at most.

Every figure is printed before it is asserted (pytest -s)."""
import contextlib
import itertools

import numpy as np
import pytest

from tests import cases
from tests import topo_reference as R

pytestmark = pytest.mark.gpu

ALL = R.NAMES
B_TERM = 2.4e-7
LAST_TILED = 3456           # 2 * 3456 floats of sine / cosine and four [64][33] blocks are 60 KB of LDS


class topo_wide:
    """hz_debug_set("topo_wide", 1) for the block, restored afterwards."""

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"topo_wide", 1))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(b"topo_wide", 0))
        return False


def _paths(hip, azim, hori, tilt, names):
    """(label, {name: map}) of every entry point that yields some of `names`."""
    T = hip.topo_param
    single = {}
    if "svf" in names:
        single["svf"] = T.sky_view_factor(azim, hori, tilt)
    if "vsf" in names:
        single["vsf"] = T.visible_sky_fraction(azim, hori, tilt)
    if "openness" in names:
        single["openness"] = T.topographic_openness(azim, hori)
    yield "single", single
    for k in range(1, len(names) + 1):
        if k == 2 or k == len(names):
            for sub in itertools.combinations(names, k):
                yield "+".join(sub), T.topo_parameters(azim, hori, tilt, which=sub)


def _cut(res, sl):
    return R.Result(res.contract[sl], res.exact[sl], res.agg_max[sl], res.scale)


class Holder:
    """Collects the comparisons of one case, prints one line per (form, output) and fails at the end with all misses."""

    def __init__(self, label, ref, per, steep):
        self.label, self.ref, self.per, self.steep = label, ref, per, steep
        self.miss, self.seen = [], {}

    def hold(self, form, wide, path, name, got, sl=None):
        ref = self.ref[name] if sl is None else _cut(self.ref[name], sl)
        where = "%s %s %s %s" % (self.label, form, path, name)
        if got.dtype != np.float32 or got.shape != ref.contract.shape:
            self.miss.append("%s: dtype / shape %s %s" % (where, got.dtype, got.shape))
            return
        nan = np.isnan(ref.contract)
        if not np.array_equal(np.isnan(got), nan):
            self.miss.append("%s: NaN in %d cells, the reference in %d" % (where, int(np.isnan(got).sum()), int(nan.sum())))
            return
        ok = ~nan
        n = int(ok.sum())
        key = (form, name)
        if name == "openness":
            bad = int((got[ok] != ref.contract[ok]).sum())
            self.seen[key] = max(self.seen.get(key, 0), bad)
            if bad:
                self.miss.append("%s: %d cells differ from the contract" % (where, bad))
        elif wide:
            per = self.per[name] if sl is None else _cut(self.per[name], sl)
            share = float((per.contract[ok] != ref.contract[ok]).mean()) if n else 0.0
            allowed = int(max(10.0 * share, 1.0e-4) * n)
            differ = ok & (got != ref.contract)
            bad = int(differ.sum())
            step = np.spacing(ref.agg_max).astype(np.float64) * ref.scale + np.spacing(np.abs(ref.contract)).astype(np.float64)
            far = int((np.abs(got.astype(np.float64) - ref.contract)[differ] > step[differ]).sum())
            self.seen[key] = max(self.seen.get(key, 0), bad)
            self.seen[(form, name, "allowed")] = "%d of %d (perturbed on the CPU: %.2g)" % (allowed, n, share)
            if bad > allowed or far:
                self.miss.append("%s: %d cells differ from the contract (allowed %d), %d by more than an ulp of the sum"
                                 % (where, bad, allowed, far))
        else:
            e_ref = R.e_ref(ref)
            bar = (2.0 if self.steep else 1.0) * e_ref + B_TERM
            err = np.abs(got.astype(np.float64) - ref.exact)
            err = float(err[ok & np.isfinite(ref.exact)].max()) if n else 0.0
            self.seen[key] = max(self.seen.get(key, 0.0), err)
            self.seen[(form, name, "allowed")] = "%.3g (E_ref %.3g%s)" % (bar, e_ref, ", steep" if self.steep else "")
            if not err <= bar:
                at = np.unravel_index(np.nanargmax(np.where(ok, np.abs(got.astype(np.float64) - ref.exact), -1.0)), got.shape)
                self.miss.append("%s: max |gpu - exact| %.3g > %.3g (E_ref %.3g) at cell %s" % (where, err, bar, e_ref, at))

    def done(self):
        for key in sorted(k for k in self.seen if len(k) == 2):
            print("TOPOREF %-34s %-5s %-8s %-10s allowed %s" % (self.label, key[0], key[1],
                  ("%.3g" % self.seen[key]) if isinstance(self.seen[key], float) else self.seen[key],
                  self.seen.get(key + ("allowed",), "0")))
        assert not self.miss, "\n".join(self.miss)


def _check(hip, label, azim, hori, tilt, names=ALL):
    ref = R.topo_reference(azim, hori, tilt, which=names)
    tilted = [n for n in names if n != "openness"]
    per = R.topo_reference(azim, hori, tilt, which=tilted, perturb_ulps=2, seed=1) if tilted else {}
    h = Holder(label, ref, per, steep=bool(tilted) and R.max_slope_deg(tilt) > 70.0)
    for form in ("tiled", "wide"):
        with topo_wide() if form == "wide" else contextlib.nullcontext():
            for path, maps in _paths(hip, azim, hori, tilt, names):
                for name, got in maps.items():
                    h.hold(form, form == "wide" or len(azim) > LAST_TILED, path, name, got)
    h.done()


@pytest.mark.parametrize("ncell", (1, 63, 64, 65, 255, 256, 257, 1025))
def test_cell_counts(hip, ncell):
    """One lane, a last wave with 63 / 1 rows, a full wave, a full workgroup and one cell more, a last workgroup with idle
    waves; 33 azimuths are one full block of the tile and one column of the next."""
    rng = np.random.default_rng(1000 + ncell)
    shape, A = R.grid_shape(ncell), 33
    _check(hip, "cells=%d A=33" % ncell, R.make_azim(A), R.hori_uniform(rng, shape, A), R.tilt_slopes(rng, shape, 70.0))


def test_map_of_many_workgroups(hip):
    rng = np.random.default_rng(7006)
    shape, A = (700, 600), 36
    _check(hip, "cells=700x600 A=36", R.make_azim(A), R.hori_uniform(rng, shape, A), R.tilt_slopes(rng, shape, 70.0))


@pytest.mark.parametrize("A", (2, 31, 32, 33, 64, 65, 90, 360, 1440, 3456, 3457, 5000))
def test_azimuth_counts(hip, A):
    """Partial and full blocks, the last count whose table fits the LDS (3456) and the first that takes the one-lane-per-cell
    kernels by itself (3457, the knob off: held to the bars of those kernels), and one well beyond."""
    rng = np.random.default_rng(2000 + A)
    shape = R.grid_shape(257 if A <= 360 else 130)
    _check(hip, "cells=%d A=%d" % (shape[0] * shape[1], A), R.make_azim(A, start=0.0 if A % 2 else 0.37),
           R.hori_uniform(rng, shape, A), R.tilt_slopes(rng, shape, 70.0))


def test_one_azimuth_openness_only(hip):
    rng = np.random.default_rng(3)
    shape = (5, 205)
    _check(hip, "cells=1025 A=1", R.make_azim(1), R.hori_uniform(rng, shape, 1), None, names=("openness",))


TILTS = {"up": lambda rng, shape: R.tilt_up(shape),
         "le35": lambda rng, shape: R.tilt_slopes(rng, shape, 35.0),
         "le70": lambda rng, shape: R.tilt_slopes(rng, shape, 70.0),
         "le89.5": lambda rng, shape: R.tilt_slopes(rng, shape, 89.5),
         "unnormalised": lambda rng, shape: R.tilt_slopes(rng, shape, 70.0, length=(0.5, 3.0))}


@pytest.mark.parametrize("half_pi", (False, True))
@pytest.mark.parametrize("tilt_class", sorted(TILTS))
def test_tilt_and_horizon_classes(hip, tilt_class, half_pi):
    """Horizons uniform in -30 ... 85 degrees, optionally 5 % of them exactly +-float32(pi/2); the normal (0, 0, 1), slopes
    up to 35, 70 and 89.5 degrees with aspects over the full circle, and vectors of length 0.5 ... 3 (the formulas take the
    raw components); azimuths that start at 0.37 radian."""
    rng = np.random.default_rng(sum(map(ord, tilt_class)) + 17 * half_pi)
    shape, A = (5, 205), 90
    hori = R.hori_uniform(rng, shape, A, frac_half_pi=0.05 if half_pi else 0.0)
    _check(hip, "tilt=%s half_pi=%d A=90" % (tilt_class, half_pi), R.make_azim(A, start=0.37), hori,
           TILTS[tilt_class](rng, shape))


def test_nan_horizons_do_not_leak(hip):
    """One NaN entry in 2 % of the cells and three whole rows of NaN: the NaN pattern of every output is the reference's
    (a NaN entry fails the comparison with the plane's horizon, which is then taken: SVF and VSF stay numbers, openness
    does not), and every other cell -- 64 cells share a wave's LDS tile -- meets the bars it meets without them."""
    rng = np.random.default_rng(77)
    shape, A = (40, 50), 45
    hori = R.add_nans(rng, R.hori_uniform(rng, shape, A), frac_cells=0.02, rows=(0, 17, 39))
    assert np.isnan(hori).any(axis=2).sum() > 150
    _check(hip, "NaN cells=40x50 A=45", R.make_azim(A), hori, R.tilt_slopes(rng, shape, 70.0))


def test_upright_plane(hip):
    """tz == 0 (and a tz so small that the squared tangent overflows float32): the tangent of the plane's own horizon is
    +-inf where the two quotients do not cancel, its arctangent +-pi/2, and the reference's result a number; where they
    cancel it is NaN.  Azimuths in one quadrant, so that whole cells stay numbers.  (Until this test existed the tiled
    kernels formed the sine as tangent * rsq(1 + tangent^2) = inf * 0 and returned NaN where the plane hides the horizon.)"""
    rng = np.random.default_rng(9)
    shape, A = (2, 65), 40
    azim = np.linspace(0.1, 1.4, A).astype(np.float32)
    tilt = R.tilt_slopes(rng, shape, 60.0)
    sx, sy = rng.choice([-1.0, 1.0], shape), rng.choice([-1.0, 1.0], shape)
    upright = rng.random(shape) < 0.6
    tilt[..., 0] = np.where(upright, sx * rng.uniform(0.2, 1.0, shape), tilt[..., 0])
    tilt[..., 1] = np.where(upright, sy * rng.uniform(0.2, 1.0, shape), tilt[..., 1])
    tilt[..., 2] = np.where(upright, rng.choice(np.array([0.0, -0.0, 1.0e-20, -1.0e-20], np.float32), shape), tilt[..., 2])
    hori = R.hori_uniform(rng, shape, A)
    ref = R.topo_reference(azim, hori, tilt, which="vsf")["vsf"].contract
    hidden = upright & ~np.isnan(ref) & (ref < 1e-6)
    assert hidden.sum() >= 10 and np.isnan(ref).sum() >= 10          # cells the plane hides entirely, cells that cancel
    _check(hip, "upright tz=0 A=40", azim, hori, tilt)


def _terrain_case(seed=41, n0=60, n1=72):
    g = cases.rough_terrain(n0, n1, seed=seed, offset=4, tilt_frames=True)
    kw = cases.grid_kwargs(g)
    tilt, *_ = cases.terrain_inputs(g)
    in0, in1 = kw["vec_norm"].shape[:2]
    mask = (np.random.default_rng(seed).random((in0, in1)) < 0.85).astype(np.uint8)
    mask[10:14, 20:30] = 0
    return kw, tilt, dict(dist_search=2.0, elev_ang_low_lim=-40.0, mask=mask, hori_fill=-0.25)


def test_maps_of_the_horizon_call(hip):
    """Real horizons of rough terrain with masked cells (hori_fill = -0.25): the maps reduced inside the horizon call --
    with the horizon returned, with topo_only=True, and for a row slab -- against the reference on the returned horizon."""
    kw, tilt, par = _terrain_case()
    par = dict(par, azim_num=36)
    G = hip.horizon.horizon_gridded
    hori, azim = G(**kw, **par)
    assert (hori == np.float32(-0.25)).all(axis=2).sum() >= 40
    ref = R.topo_reference(azim, hori, tilt)
    per = R.topo_reference(azim, hori, tilt, which=("svf", "vsf"), perturb_ulps=2, seed=1)
    h = Holder("horizon call 52x64 A=36", ref, per, steep=R.max_slope_deg(tilt) > 70.0)
    rb, re = 9, 30
    for form in ("tiled", "wide"):
        with topo_wide() if form == "wide" else contextlib.nullcontext():
            h2, a2, maps = G(**kw, **par, topo=ALL, topo_vec_tilt=tilt)
            assert np.array_equal(h2, hori) and np.array_equal(a2, azim)
            none, _, only = G(**kw, **par, topo=ALL, topo_vec_tilt=tilt, topo_only=True)
            assert none is None
            _, _, slab = G(**kw, **par, topo=ALL, topo_vec_tilt=tilt, topo_only=True, rows=(rb, re), _chunk_rows=5)
            _, _, svf = G(**kw, **par, svf_vec_tilt=tilt)
        h.hold(form, form == "wide", "svf_vec_tilt", "svf", svf)
        for name in ALL:
            h.hold(form, form == "wide", "topo=", name, maps[name])
            h.hold(form, form == "wide", "topo_only", name, only[name])
            assert np.isnan(slab[name][:rb]).all() and np.isnan(slab[name][re:]).all()
            h.hold(form, form == "wide", "rows", name, slab[name][rb:re], sl=slice(rb, re))
    h.done()


def test_horizon_array_beyond_2_to_32_elements(hip):
    """3569 x 3400 cells x 360 azimuths = 4.37e9 floats (17.5 GB; the headline tile has 3569^2): `hori` is filled on the
    device from the closed-form pattern of tests/topo_reference.py, hz_topo_params runs on device pointers, and 2000-odd
    sampled cells -- the first, the last, the last workgroups, the cells either side of element 2^32 -- are compared with
    the reference evaluated on the same pattern."""
    import torch
    from horayzon_amd import _lib
    L = _lib.lib()
    n0, n1, A, seed = 3569, 3400, 360, 12345
    ncell = n0 * n1
    assert ncell * A > 2 ** 32
    free, _ = torch.cuda.mem_get_info(0)
    if free < 40e9:
        pytest.skip("needs 40 GB of free device memory for a 17.5 GB horizon array, %.1f GB are free" % (free / 1e9))
    rng = np.random.default_rng(seed)
    azim = R.make_azim(A)
    tilt = R.tilt_slopes(rng, (ncell,), 60.0)
    edge = 2 ** 32 // A                                       # the cell that holds element 2^32
    cells = np.unique(np.concatenate([np.arange(0, 70), np.arange(ncell - 300, ncell), np.arange(edge - 70, edge + 70),
                                      rng.integers(0, ncell, 1600)])).astype(np.int64)
    hori_s = R.pattern_hori(cells[:, None], np.arange(A, dtype=np.int64)[None, :], seed)[None]
    assert hori_s.dtype == np.float32 and -0.5 <= hori_s.min() < -0.49 and 1.49 < hori_s.max() < 1.5
    tilt_s = np.ascontiguousarray(tilt[cells])[None]
    ref = R.topo_reference(azim, hori_s, tilt_s)
    per = R.topo_reference(azim, hori_s, tilt_s, which=("svf", "vsf"), perturb_ulps=2, seed=1)
    h = Holder("2^32 elements, %d sampled cells" % len(cells), ref, per, steep=False)
    dev = torch.device("cuda:0")
    d_hori = d_tilt = d_out = None
    try:
        d_hori = torch.empty((ncell, A), dtype=torch.float32, device=dev)
        k = torch.arange(A, dtype=torch.int64, device=dev)[None, :]
        step = 1 << 18
        for c0 in range(0, ncell, step):
            c1 = min(ncell, c0 + step)
            d_hori[c0:c1] = R.pattern_hori(torch.arange(c0, c1, dtype=torch.int64, device=dev)[:, None], k, seed, xp=torch)
        d_cells = torch.from_numpy(cells).to(dev)
        assert np.array_equal(d_hori[d_cells].cpu().numpy(), hori_s[0])      # both sides reduce the same numbers
        d_tilt = torch.from_numpy(tilt).to(dev)
        d_out = torch.empty((3, ncell), dtype=torch.float32, device=dev)
        ptrs = [d_out[i].data_ptr() for i in range(3)]
        for form in ("tiled", "wide"):
            for path, want in (("svf+vsf+openness", (1, 1, 1)), ("svf", (1, 0, 0))) if form == "tiled" else \
                    (("svf+vsf+openness", (1, 1, 1)),):
                d_out.fill_(float("nan"))
                torch.cuda.synchronize()
                with topo_wide() if form == "wide" else contextlib.nullcontext():
                    _lib.check(L.hz_topo_params(azim.ctypes.data, d_hori.data_ptr(), d_tilt.data_ptr(), n0, n1, A,
                                                *[p if w else None for p, w in zip(ptrs, want)], 0))
                torch.cuda.synchronize()
                got = d_out[:, d_cells].cpu().numpy()
                for i, name in enumerate(ALL):
                    if want[i]:
                        h.hold(form, form == "wide", path, name, got[i][None])
    finally:
        del d_hori, d_tilt, d_out
        torch.cuda.empty_cache()
    h.done()
