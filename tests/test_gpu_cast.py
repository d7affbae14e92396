"""Terrain.cast on the GPU: every case word for word (uint32 views, NaN positions included) against the CPU yardstick
(tests/cast_reference.py: the NumPy float32 rays and the oracle's any-hit and closest-hit answers with a tfar per ray) --
the bytes, the distances, the hit points and the number of rays -- and against Terrain.panorama and Terrain.viewshed,
whose rays a cast can restate.  Outputs are filled with junk first, so an element that is not written shows."""
import itertools

import numpy as np
import pytest

from tests import cast_reference as cr
from tests import panorama_reference as pr
from tests import viewshed_reference as vr
from tests.test_cast_reference import BLOCKED, DEGENERATE, HITS, MAX_DIST, N, SEED_RAYS, SEED_SEGMENTS, SHORT_DIST
from tests.test_panorama_reference import angles, six_observers
from tests.test_viewshed_reference import fixture

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257, N)          # partial waves, one wave, one ray more, a partial workgroup, many workgroups
SUBSETS = [w for w in itertools.product((False, True), repeat=3) if any(w)]       # (occluded, dist, point)
JUNK = np.float32(-77.25)


class knob:
    """hz_debug_set(key, value) for the block, the default restored afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key.encode(), value

    def __enter__(self):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, self.value))

    def __exit__(self, *exc):
        from horayzon_amd import _lib
        _lib.check(_lib.lib().hz_debug_set(self.key, -1))
        return False


def buffers(n, want, torch=None, dev=None):
    """(occluded, dist, point) filled with junk, None where not wanted; NumPy, or tensors on `dev`."""
    if torch is None:
        return (np.full(n, 77, np.uint8) if want[0] else None, np.full(n, JUNK, np.float32) if want[1] else None,
                np.full((n, 3), JUNK, np.float32) if want[2] else None)
    return (torch.full((n,), 77, dtype=torch.uint8, device=dev) if want[0] else None,
            torch.full((n,), float(JUNK), dtype=torch.float32, device=dev) if want[1] else None,
            torch.full((n, 3), float(JUNK), dtype=torch.float32, device=dev) if want[2] else None)


def run(t, org, ends, mode, max_dist=MAX_DIST, want=(True, True, True), **kw):
    """(occluded, dist, point, stats) of a call with NumPy outputs."""
    occ, dist, point = buffers(org.shape[0], want)
    if mode == "directions":
        t.cast(org, ends, max_dist=max_dist, occluded=occ, dist=dist, point=point, **kw)
    else:
        t.cast(org, targets=ends, occluded=occ, dist=dist, point=point, **kw)
    return occ, dist, point, dict(t.last_stats)


def check(got, ref, n=None):
    """`ref` = (occluded, dist, point, live) of the whole set; the first n rays of it are compared."""
    occ, dist, point, st = got
    occ_ref, dist_ref, point_ref, live = ref
    n = occ_ref.shape[0] if n is None else n
    occ_ref, dist_ref, point_ref, rays = occ_ref[:n], dist_ref[:n], point_ref[:n], int(live[:n].sum())
    print("rays %d / %d, bytes differing %s, dist words differing %s, point words differing %s" % (
        st["num_rays"], rays, None if occ is None else int((occ != occ_ref).sum()),
        None if dist is None else int((cr.words(dist) != cr.words(dist_ref)).sum()),
        None if point is None else int((cr.words(point) != cr.words(point_ref)).sum())))
    for name, a, b in (("dist", dist, dist_ref), ("point", point, point_ref)):
        if a is not None and a.shape == b.shape:
            for idx in np.argwhere(cr.words(a) != cr.words(b))[:8]:
                print("  %s%s: %r (0x%08x), reference %r (0x%08x)" % (name, tuple(int(i) for i in idx), float(a[tuple(idx)]),
                                                                    int(cr.words(a)[tuple(idx)]), float(b[tuple(idx)]), int(cr.words(b)[tuple(idx)])))
    if occ is not None:
        assert occ.dtype == np.uint8 and occ.shape == occ_ref.shape and np.array_equal(occ, occ_ref)
    if dist is not None:
        assert dist.shape == dist_ref.shape and np.array_equal(cr.words(dist), cr.words(dist_ref))
    if point is not None:
        assert point.shape == point_ref.shape and np.array_equal(cr.words(point), cr.words(point_ref))
    assert st["num_rays"] == rays


class Small:
    """The 40 x 40 fixture of the CPU tests, a Terrain, the two seeded ray sets and their references, each computed once."""

    def __init__(self, hip):
        from oracle import oracle as orc
        self.g, *self.arrays = fixture()
        vec_tilt, vec_norm, enl, elev, mask = self.arrays
        g = self.g
        self.t = hip.shadow.Terrain()
        self.t.initialise(g["vert_grid"], g["dem_dim_0"], g["dem_dim_1"], g["offset_0"], g["offset_1"], vec_tilt, vec_norm, enl, elev, mask)
        self.scene = orc.Scene(g["vert_grid"], 40, 40)
        self.sets = {"directions": cr.random_rays(g, N, SEED_RAYS),
                     "targets": cr.random_segments(g["vert_grid"], 40, 40, N, SEED_SEGMENTS)}
        self.refs = {}

    def ref(self, mode, max_dist=MAX_DIST):
        key = (mode, max_dist if mode == "directions" else None)
        if key not in self.refs:
            org, ends = self.sets[mode]
            kw = dict(directions=ends, max_dist=max_dist) if mode == "directions" else dict(targets=ends)
            occ, dist, point, _ = cr.cast(self.g["vert_grid"], 40, 40, org, scene=self.scene, **kw)
            live = cr.rays(org, **kw)[3]
            for a in (occ, dist, point, live):
                a.setflags(write=False)
            self.refs[key] = (occ, dist, point, live)
        return self.refs[key]


@pytest.fixture(scope="module")
def small(hip):
    return Small(hip)


def test_the_sets_are_the_pinned_ones(small):
    assert int(small.ref("directions")[0].sum()) == HITS[MAX_DIST] and int(small.ref("directions", SHORT_DIST)[0].sum()) == HITS[SHORT_DIST]
    occ, _, _, live = small.ref("targets")
    assert int(occ.sum()) == BLOCKED and int((~live).sum()) == DEGENERATE > 0


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("mode", ("directions", "targets"))
def test_ray_counts_and_every_subset_of_the_outputs(small, mode, n):
    """occluded alone runs k_cast_any, every subset with dist or point k_cast_closest: the words do not depend on it."""
    org, ends = (np.ascontiguousarray(a[:n]) for a in small.sets[mode])
    for want in SUBSETS:
        check(run(small.t, org, ends, mode, want=want), small.ref(mode), n)


def test_short_rays(small):
    org, ends = small.sets["directions"]
    for want in ((True, False, False), (True, True, True)):
        check(run(small.t, org, ends, "directions", SHORT_DIST, want), small.ref("directions", SHORT_DIST))


@pytest.mark.parametrize("mode", ("directions", "targets"))
def test_same_byte_from_both_kernels(small, mode):
    org, ends = small.sets[mode]
    any_hit = run(small.t, org, ends, mode, want=(True, False, False))
    closest = run(small.t, org, ends, mode, want=(True, True, False))
    assert np.array_equal(any_hit[0], closest[0])
    assert np.array_equal(closest[0].astype(bool), ~np.isnan(closest[1]))
    assert 0 < int(any_hit[0].sum()) < N
    assert any_hit[3]["num_rays"] == closest[3]["num_rays"] == int(small.ref(mode)[3].sum())


@pytest.mark.parametrize("mode", ("directions", "targets"))
def test_chunks_give_the_words_of_one_chunk(small, mode):
    """`cast_budget` cuts the 4099 rays into chunks of 1024 with a last one of 3; the memory reported is that of a chunk and
    does not grow with the number of rays."""
    torch = pytest.importorskip("torch")
    t = small.t
    org, ends = small.sets[mode]
    ref = small.ref(mode)
    dev = "cuda:%d" % t.device
    whole = run(t, org, ends, mode)
    check(whole, ref)
    assert whole[3]["scratch_bytes"] == 4160 * 41            # one chunk of 65 waves: two inputs of 12 bytes, 1 + 4 + 12 of outputs
    twice = tuple(np.ascontiguousarray(np.vstack([a, a])) for a in (org, ends))
    ref2 = tuple(np.concatenate([a, a]) for a in ref)
    with knob("cast_budget", 41 * 1024 + 40):
        got = run(t, org, ends, mode)
        check(got, ref)
        assert got[3]["scratch_bytes"] == 1024 * 41
        got2 = run(t, *twice, mode)
        check(got2, ref2)
        assert got2[3]["scratch_bytes"] == got[3]["scratch_bytes"]
        # occluded alone: the any-hit kernel in chunks of 1024 * 41 / 25 -> 1664 rays
        got = run(t, org, ends, mode, want=(True, False, False))
        check(got, ref)
        assert got[3]["scratch_bytes"] == 1664 * 25
    # one wave per chunk
    with knob("cast_budget", 1):
        check(run(t, org[:257], ends[:257], mode), ref, 257)
        assert t.last_stats["scratch_bytes"] == 64 * 41
    # tensors in and out: nothing is staged and the budget plays no part -- until the sort needs its 16 bytes per ray
    d_org, d_ends = torch.from_numpy(org).to(dev), torch.from_numpy(ends).to(dev)
    kw = dict(max_dist=MAX_DIST) if mode == "directions" else {}
    for order, scratch in (("given", 0), ("sorted", None)):
        with knob("cast_budget", 16 * 1024):
            occ, dist, point = buffers(N, (True, True, True), torch, dev)
            torch.cuda.synchronize()
            t.cast(d_org, **{mode: d_ends}, occluded=occ, dist=dist, point=point, order=order, **kw)
            torch.cuda.synchronize()
            st = dict(t.last_stats)
        check((occ.cpu().numpy(), dist.cpu().numpy(), point.cpu().numpy(), st), ref)
        if scratch is not None:
            assert st["scratch_bytes"] == scratch
        else:
            assert 16 * 1024 <= st["scratch_bytes"] <= 16 * 1024 + 64 * 1024        # the sort's histograms on top
            sorted_bytes = st["scratch_bytes"]
            occ2, dist2, point2 = buffers(2 * N, (True, True, True), torch, dev)
            with knob("cast_budget", 16 * 1024):
                t.cast(torch.cat([d_org, d_org]), **{mode: torch.cat([d_ends, d_ends])}, occluded=occ2, dist=dist2, point=point2,
                       order=order, **kw)
                torch.cuda.synchronize()
            check((occ2.cpu().numpy(), dist2.cpu().numpy(), point2.cpu().numpy(), dict(t.last_stats)), ref2)
            assert t.last_stats["scratch_bytes"] == sorted_bytes


@pytest.mark.parametrize("mode", ("directions", "targets"))
def test_sorted_order_gives_the_words_of_the_given_order(small, mode):
    t = small.t
    org, ends = small.sets[mode]
    ref = small.ref(mode)
    perm = np.random.default_rng(23).permutation(N)
    shuffled = (np.ascontiguousarray(org[perm]), np.ascontiguousarray(ends[perm]))
    ref_shuffled = tuple(np.ascontiguousarray(a[perm]) for a in ref)
    for want in ((True, True, True), (True, False, False), (False, True, False)):
        check(run(t, org, ends, mode, want=want, order="sorted"), ref)
        check(run(t, *shuffled, mode, want=want, order="given"), ref_shuffled)
        check(run(t, *shuffled, mode, want=want, order="sorted"), ref_shuffled)
        # the sort is per chunk: 57 (41 for occluded alone: 12 + 12 + 1 + 16) bytes per ray, chunks of 1024 and a last one of 3
        with knob("cast_budget", (57 if want[1] or want[2] else 41) * 1024):
            for a, b in ((org, ends), shuffled):
                got = run(t, a, b, mode, want=want, order="sorted")
                check(got, ref if a is org else ref_shuffled)
                assert got[3]["scratch_bytes"] < 1024 * 57 + 64 * 1024
    for n in (1, 64, 65):
        check(run(t, org[:n].copy(), ends[:n].copy(), mode, order="sorted"), ref, n)


@pytest.mark.parametrize("mode", ("directions", "targets"))
def test_tensors_in_and_out_equal_the_numpy_call(small, mode):
    torch = pytest.importorskip("torch")
    t = small.t
    org, ends = small.sets[mode]
    ref = small.ref(mode)
    dev = "cuda:%d" % t.device
    d_org, d_ends = torch.from_numpy(org).to(dev), torch.from_numpy(ends).to(dev)
    kw = dict(max_dist=MAX_DIST) if mode == "directions" else {}
    for want in SUBSETS:
        occ, dist, point = buffers(N, want, torch, dev)
        torch.cuda.synchronize()
        t.cast(d_org, **{mode: d_ends}, occluded=occ, dist=dist, point=point, **kw)
        torch.cuda.synchronize()
        st = dict(t.last_stats)
        assert st["scratch_bytes"] == 0
        check(tuple(None if b is None else b.cpu().numpy() for b in (occ, dist, point)) + (st,), ref)
    # one input and one output on each side
    occ, dist, point = buffers(N, (True, True, True))
    d_dist = torch.full((N,), float(JUNK), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t.cast(org, **{mode: d_ends}, occluded=occ, dist=d_dist, point=point, **kw)
    torch.cuda.synchronize()
    check((occ, d_dist.cpu().numpy(), point, dict(t.last_stats)), ref)
    assert t.last_stats["scratch_bytes"] == 4160 * (12 + 1 + 12)
    t.cast(d_org, **{mode: ends}, dist=d_dist, **kw)
    torch.cuda.synchronize()
    check((None, d_dist.cpu().numpy(), None, dict(t.last_stats)), ref)


def test_staged_and_device_outputs_in_one_chunked_call(small):
    """Chunks of 1024 rays and a last one of 3, with `occluded` and `point` staged anew for every chunk and `dist` a tensor
    written in place at the chunk's offset."""
    torch = pytest.importorskip("torch")
    t = small.t
    org, ends = small.sets["targets"]
    dev = "cuda:%d" % t.device
    occ, _, point = buffers(N, (True, False, True))
    d_dist = torch.full((N,), float(JUNK), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with knob("cast_budget", 25 * 1024 + 24):               # staged per ray: 12 of origins, 1 of occluded, 12 of point
        t.cast(org, targets=torch.from_numpy(ends).to(dev), occluded=occ, dist=d_dist, point=point)
    torch.cuda.synchronize()
    check((occ, d_dist.cpu().numpy(), point, dict(t.last_stats)), small.ref("targets"))
    assert t.last_stats["scratch_bytes"] == 1024 * 25


def test_panoramas_rays_give_the_panoramas_words(small):
    """cast(directions = the panorama's rays) is Terrain.panorama's dist and point, the observer on a vertex included."""
    t, g = small.t, small.g
    obs = six_observers(g)
    azim, elev = angles(45, 21)
    dirs = pr.rays(obs, azim, elev)
    org = np.ascontiguousarray(np.broadcast_to(obs[:, None, None, :], dirs.shape)).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs.reshape(-1, 3))
    for max_dist in (MAX_DIST, SHORT_DIST):
        p_dist = np.full((6, 21, 45), JUNK, np.float32)
        p_point = np.full((6, 21, 45, 3), JUNK, np.float32)
        hits = np.zeros(6, np.int64)
        t.panorama(obs, azim, elev, max_dist, dist=p_dist, point=p_point, hits=hits)
        occ, dist, point, st = run(t, org, dirs, "directions", max_dist)
        assert np.array_equal(cr.words(dist), cr.words(p_dist.reshape(-1)))
        assert np.array_equal(cr.words(point), cr.words(p_point.reshape(-1, 3)))
        assert np.array_equal(occ.reshape(6, -1).sum(axis=1), hits) and st["num_rays"] == 6 * 21 * 45
        assert (cr.words(dist.reshape(6, -1)[5]) == 0).all()              # on the vertex: +0.0 in every direction
        only = run(t, org, dirs, "directions", max_dist, want=(True, False, False))
        assert np.array_equal(only[0], occ)


def test_viewsheds_segments_give_the_viewsheds_codes(small):
    """cast(origins = the viewshed's target points, targets = the observer) is occluded exactly where viewshed(facing=False)
    says blocked, wherever it gives 0 or 2."""
    t, g = small.t, small.g
    vec_tilt, vec_norm, enl, elev, mask = small.arrays
    obs = six_observers(g)
    in0, in1 = mask.shape
    v = vr.vertices(g["vert_grid"], 40, 40)[g["offset_0"]:g["offset_0"] + in0, g["offset_1"]:g["offset_1"] + in1]
    target = (v + np.ascontiguousarray(vec_norm, np.float32) * np.float32(0.05)).astype(np.float32).reshape(-1, 3)
    codes = np.full((6, in0, in1), 77, np.uint8)
    t.viewshed(obs, visible=codes, facing=False)
    assert set(np.unique(codes)) <= {0, 2, 3} and (codes == 0).sum() > 100 and (codes == 2).sum() > 100
    for s in range(6):
        ends = np.ascontiguousarray(np.broadcast_to(obs[s], target.shape))
        for want in ((True, False, False), (True, True, False)):
            occ = run(t, np.ascontiguousarray(target), ends, "targets", want=want)[0]
            ray = (codes[s].reshape(-1) == 0) | (codes[s].reshape(-1) == 2)
            assert np.array_equal(occ[ray] == 1, codes[s].reshape(-1)[ray] == 2), s


@pytest.mark.parametrize("mode", ("directions", "targets"))
def test_overflowed_rays_are_traced_again(small, mode):
    """The in-kernel retry of k_cast_any: with as few fast-stack entries as the launcher accepts (>= 5 and >= the tree's
    height) many rays run out of entries and are traced again with the level stack -- with their own tfar.  That the retry
    ran shows in the node visits: a ray traced twice visits the nodes of both traversals.  The level stack alone (cap 0)
    and the counting instantiations give the same bytes."""
    t = small.t
    org, ends = small.sets[mode]
    ref = small.ref(mode)
    want = (True, False, False)
    check(run(t, org, ends, mode, want=want), ref)
    height = t.last_stats["bvh_height"]
    cap = max(5, height)
    assert height >= 1 and cap < 19
    print("bvh_height %d, cap %d" % (height, cap))
    with knob("cast_fast_cap", cap):
        check(run(t, org, ends, mode, want=want), ref)
    with knob("cast_fast_cap", 0):
        check(run(t, org, ends, mode, want=want), ref)
    try:
        t.count_work(True)
        default = run(t, org, ends, mode, want=want)
        check(default, ref)
        with knob("cast_fast_cap", cap):
            low = run(t, org, ends, mode, want=want)
        check(low, ref)
        with knob("cast_fast_cap", 0):
            level = run(t, org, ends, mode, want=want)
        check(level, ref)
    finally:
        t.count_work(False)
    print("nodes visited: default cap %d, cap %d: %d, level stack %d" % (
        default[3]["nodes_visited"], cap, low[3]["nodes_visited"], level[3]["nodes_visited"]))
    assert default[3]["nodes_visited"] > 0 and default[3]["tris_tested"] > 0
    assert low[3]["nodes_visited"] > default[3]["nodes_visited"]
    got = run(t, org, ends, mode, want=want)
    check(got, ref)
    assert got[3]["nodes_visited"] == 0
