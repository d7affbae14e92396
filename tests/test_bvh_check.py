"""tests/bvh_check.py checked where there is no GPU: blobs of its plain-Python reference builder are valid, and every
defect of the list in bvh_check.mutations, applied to a host copy, is reported under its kind -- without the checker
raising or looping (one mutation links a node back to the root's block)."""
import numpy as np
import pytest

from tests import bvh_check


_grid = bvh_check.plain_grid


GRIDS = {
    "2x2": lambda: _grid(2, 2, relief=40.0),
    "2x3": lambda: _grid(2, 3, relief=40.0),
    "3x3": lambda: _grid(3, 3, relief=40.0),
    "5x7 random relief": lambda: _grid(5, 7, relief=300.0),
    "flat 6x6": lambda: _grid(6, 6),
    "4x9 at (2.6e6, 1.2e6)": lambda: _grid(4, 9, relief=100.0, origin=(2.6e6, 1.2e6), dx=1.0),
}


def _show(findings):
    return "\n".join("%s[%d]: %s" % f for f in findings[:10])


@pytest.mark.parametrize("name", list(GRIDS))
def test_reference_builder_blobs_are_valid(name):
    vg, d0, d1 = GRIDS[name]()
    blob = bvh_check.build_reference(vg, d0, d1)
    stats = {}
    findings = bvh_check.check(blob, vg, d0, d1, stats=stats)
    assert findings == [], _show(findings)
    dec = bvh_check.decode(blob)
    assert dec["hdr"]["n_prims"] == (d0 - 1) * (d1 - 1) and stats["height"] == dec["hdr"]["height"]
    assert all(r >= 1.0 for r in stats["step_ratio"])         # 255 steps span every node


def test_reference_builder_makes_wrapper_nodes_on_a_cut_off_grid():
    vg, d0, d1 = GRIDS["flat 6x6"]()                         # 5 x 5 quads: quad (4, 4) is a single leaf beside three subtrees
    dec = bvh_check.decode(bvh_check.build_reference(vg, d0, d1))
    q = dec["nodes"]["q"]
    present = ~((q[:, 8::2] == 255) & (q[:, 9::2] == 0))
    dead = np.array([n.tobytes() == bvh_check.DEAD_BYTES for n in dec["nodes"]])
    assert ((present.sum(axis=1) == 1) & ~dead)[1:].any()


_MUT = {}


def _mutations():
    if not _MUT:
        vg, d0, d1 = GRIDS["5x7 random relief"]()
        blob = bvh_check.build_reference(vg, d0, d1)
        assert bvh_check.check(blob, vg, d0, d1) == []
        _MUT.update(inputs=(vg, d0, d1), muts=bvh_check.mutations(blob))
    return _MUT


MUTATION_NAMES = ["upper code one smaller", "lower code one larger", "upper code one larger",
                  "two leaf records of different blocks swapped", "one leaf record copied over another",
                  "first moved by 2", "first set to 0 (a cycle)", "live child replaced by the dead pattern",
                  "dead slot zeroed", "x-step exponent bits of one origin incremented", "one anc entry changed",
                  "height decremented", "one vertex word changed", "pad halved"]


def test_mutation_list_is_complete():
    assert [m[0] for m in _mutations()["muts"]] == MUTATION_NAMES


@pytest.mark.parametrize("name", MUTATION_NAMES)
def test_mutation_is_reported_under_its_kind(name):
    m = _mutations()
    _, kinds, blob = next(x for x in m["muts"] if x[0] == name)
    findings = bvh_check.check(blob, *m["inputs"])
    got = {f.kind for f in findings}
    assert "internal" not in got, _show(findings)
    assert got & set(kinds), "%s: expected %s, got\n%s" % (name, kinds, _show(findings))


def test_a_wrapper_that_lost_its_parents_pair_is_a_box_finding():
    vg, d0, d1 = GRIDS["flat 6x6"]()
    blob = bvh_check.build_reference(vg, d0, d1)
    dec = bvh_check.decode(blob)
    q = dec["nodes"]["q"]
    present = ~((q[:, 8::2] == 255) & (q[:, 9::2] == 0))
    w = int(np.flatnonzero((present.sum(axis=1) == 1) & (np.arange(q.shape[0]) > 3))[0])
    off = dec["hdr"]["off_nodes"] + 32 * w
    for byte, by in ((17, 1), (19, 1), (0, 0x200)):          # x pair made wider (still covers), the empty pair filled, origin moved
        b = blob.copy()
        if byte == 0:
            b[off:off + 4].view("<u4")[0] += by
        else:
            b[off + byte] = np.uint8(int(b[off + byte]) + by)
        assert "box" in {f.kind for f in bvh_check.check(b, vg, d0, d1)}


def _small_folded_sheet(n=20, fold=16, dx=50.0):
    """tests/test_gpu_near_guard.py's folded sheet in small, folded near its end: the rows beyond `fold` run back over
    the rows before it (the minority), so the bitmap has marked and unmarked cells."""
    vg, _, _ = bvh_check.plain_grid(n, n, relief=20.0, dx=dx, seed=7)
    i = np.arange(n)
    y = ((fold - np.abs(i - fold)) * dx).astype(np.float32)
    vg[1:3 * n * n:3].reshape(n, n)[:] = y[:, None]
    vg[2:3 * n * n:3].reshape(n, n)[i > fold] += np.float32(23.0)
    return vg, n, n


def test_bad_quad_bitmap_of_a_folded_sheet():
    """Not a height field: the reference builder marks the bad quads cell by cell, the checker rebuilds the bitmap from
    cell boxes -- they must agree bit for bit, and every defect of the bitmap or its header fields is a `badmap` finding."""
    vg, d0, d1 = _small_folded_sheet()
    blob = bvh_check.build_reference(vg, d0, d1)
    h = bvh_check.decode(blob)["hdr"]
    assert h["flags"] == bvh_check.HZ_BLOB_BAD_MAP and 0 < h["n_flipped"] < 2 * h["n_quads"]
    findings = bvh_check.check(blob, vg, d0, d1)
    assert findings == [], _show(findings)
    muts = bvh_check.badmap_mutations(blob)
    assert [m[0] for m in muts] == ["a set bitmap cell cleared", "an unset bitmap cell set", "n_flipped incremented",
                                    "HEIGHT_FIELD set beside BAD_MAP", "BAD_MAP cleared", "bad_sx scaled"]
    for name, kinds, bad in muts:
        got = {f.kind for f in bvh_check.check(bad, vg, d0, d1)}
        assert "internal" not in got and got & set(kinds), (name, got)


def test_checker_survives_garbage():
    """Truncated, zeroed and random bytes: findings, never an exception (the `internal` kind) or a hang."""
    m = _mutations()
    blob = m["muts"][0][2]
    rng = np.random.default_rng(11)
    noise = blob.copy()
    off = bvh_check.decode(blob)["hdr"]["off_nodes"]
    noise[off:] = rng.integers(0, 256, noise.size - off, dtype=np.uint8)
    for b in (blob[:100], blob[:1000], np.zeros_like(blob), noise):
        findings = bvh_check.check(b, *m["inputs"])
        assert findings and "internal" not in {f.kind for f in findings}, _show(findings)
