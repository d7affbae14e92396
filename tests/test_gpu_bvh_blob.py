"""The scene blob that hz_scene.hip builds on the device, copied to the host and held against tests/bvh_check.py: header,
topology, primitives, the containment of every leaf box in every ancestor slot box (float32 replication of the leaf
boxes and unions, float64 evaluation of the quantised planes -- exact, no tolerance), tightness of the codes, hit-cache
ancestors and the bad-quad bitmap.  The horizon / shadow suites compare results computed THROUGH this structure; a box
that is too small shows there only for a ray that enters exactly there, and everything that "cannot change a result"
(dead nodes, anc, boxes too large, height, unused bitmap cells) shows nowhere else.

Tightness as asserted is exactly what axis_lo / axis_hi (hz_scene.hip) guarantee: the lower code is 255 or the next
plane lies above lo - m, the upper code is 0 or the previous plane lies below hi + m.  Wrapper nodes are excepted: they
carry their parent's pairs (k_bfs_emit), whose x / y ranges belong to the parent's halves.

Every scene prints one JSON line (node count, leaf-slot fill, height, largest 255 * step / node extent per axis); the step
ratios are reported, not asserted -- the step depends on the embed_down retries of axis_try.

A mutated blob exists in host memory only: nothing here hands one to Scene.adopt or to a kernel."""
import json
import os

import numpy as np
import pytest

from horayzon_amd import synth
from tests import bvh_check, cases
from tests.test_gpu_near_guard import _folded_sheet

pytestmark = pytest.mark.gpu


def _dem(vert_grid, d0, d1, vs=None, ts=None):
    return dict(vert_grid=vert_grid, d0=d0, d1=d1, vs=vs, ts=ts)


def _rough(n0, n1, seed, **kw):
    g = cases.rough_terrain(n0, n1, seed=seed, **kw)
    return g, _dem(g["vert_grid"], n0, n1)


def _big():
    return cases.rough_terrain(140, 150, seed=33, relief=1200.0)


def _rotated(axis, deg):
    """The 140 x 150 vertices rotated about the world z axis (a half's x / y range becomes a union) or about x (z is
    no longer 'up': the construction of test_gpu_near_guard.py)."""
    g = _big()
    v = g["vert_grid"][:3 * 140 * 150].reshape(-1, 3).astype(np.float64)
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) if axis == "z" else \
        np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    w = (v @ rot.T).astype(np.float32)
    return _dem(synth.pack_vertices(w[:, 0].reshape(140, 150), w[:, 1].reshape(140, 150), w[:, 2].reshape(140, 150)), 140, 150)


def _face_300_to_1():
    vg, n0, n1 = bvh_check.plain_grid(40, 40, relief=2.0, origin=(-4.0e5, -4.0e5), dx=1.0, seed=5)
    vg[2:3 * 1600:3].reshape(40, 40)[20, :] += np.float32(300.0)
    return _dem(vg, 40, 40)


def _curved():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curved_dem_reference.npz"))
    n0, n1 = d["x_enu"].shape
    return _dem(synth.pack_vertices(d["x_enu"], d["y_enu"], d["z_enu"]), n0, n1)


def _folded():
    kw = _folded_sheet()
    return _dem(kw["vert_grid"], kw["dem_dim_0"], kw["dem_dim_1"])


def _outer_tin(form):
    g = _big()
    vs, nvs, ts, nts = cases.outer_tin(g)
    vs, ts = vs.reshape(-1, 3), ts.reshape(-1, 3)
    if form == "tiny":
        # 64 triangles with 1 m edges over one and the same square metre outside the DEM (inside the ring), stacked in
        # z: their centroid keys coincide, only the tie-break of delta() separates them
        x0, y0 = float(g["x"].max()) + 1500.0, float(g["y"].max()) + 1500.0
        k = np.arange(64, dtype=np.float32)
        tiny = np.stack([np.stack([np.full(64, x0), np.full(64, y0), 400.0 + 0.5 * k], axis=1),
                         np.stack([np.full(64, x0 + 1.0), np.full(64, y0), 400.0 + 0.5 * k], axis=1),
                         np.stack([np.full(64, x0), np.full(64, y0 + 1.0), 400.25 + 0.5 * k], axis=1)], axis=1)
        idx = (vs.shape[0] + np.arange(3 * 64, dtype=np.int32)).reshape(64, 3)
        vs = np.concatenate([vs, tiny.reshape(-1, 3).astype(np.float32)], axis=0)
        ts = np.concatenate([ts, idx], axis=0)
    elif form == "copies":
        ts = np.concatenate([ts, np.tile(ts[:1], (40, 1))], axis=0)
    return _dem(g["vert_grid"], 140, 150, np.ascontiguousarray(vs, np.float32).ravel(), np.ascontiguousarray(ts, np.int32).ravel())


SCENES = {
    # one and two primitives (k_single_tmp), the smallest blocks
    "2x2 flat": lambda: _dem(*bvh_check.plain_grid(2, 2)),
    "2x2 relief": lambda: _dem(*bvh_check.plain_grid(2, 2, relief=40.0)),
    "2x3": lambda: _dem(*bvh_check.plain_grid(2, 3, relief=40.0)),
    "3x2": lambda: _dem(*bvh_check.plain_grid(3, 2, relief=40.0)),
    "3x3": lambda: _dem(*bvh_check.plain_grid(3, 3, relief=40.0)),
    # flat DEMs: z extent 0
    "33x47 flat": lambda: _dem(*bvh_check.plain_grid(33, 47)),
    "33x47 flat at (2.6e6, 1.2e6), 1 m": lambda: _dem(*bvh_check.plain_grid(33, 47, origin=(2.6e6, 1.2e6), dx=1.0)),
    # strips
    "2x1500": lambda: _dem(*bvh_check.plain_grid(2, 1500, relief=300.0)),
    "1500x2": lambda: _dem(*bvh_check.plain_grid(1500, 2, relief=300.0)),
    "3x1500": lambda: _rough(3, 1500, 4, offset=0, relief=300.0)[1],
    # power-of-two boundaries of the quad grid
    "64x64": lambda: _rough(64, 64, 21)[1],
    "65x65": lambda: _rough(65, 65, 22)[1],
    "66x64": lambda: _rough(66, 64, 23)[1],
    "140x150": lambda: _dem(_big()["vert_grid"], 140, 150),
    "300:1 face at -4e5": _face_300_to_1,
    # rotated and curved grids
    "140x150 rotated 30 deg about z": lambda: _rotated("z", 30.0),
    "140x150 rotated 20 deg about x": lambda: _rotated("x", 20.0),      # (no slope of this terrain tips over: still a height field)
    "140x150 rotated 80 deg about x": lambda: _rotated("x", 80.0),      # slopes facing away project flipped: a bad map
    "curved ENU grid": _curved,
    "folded sheet": _folded,
    "outer TIN": lambda: _outer_tin("ring"),
    "outer TIN + 64 tiny triangles with one key": lambda: _outer_tin("tiny"),
    "outer TIN + 40 copies of one triangle": lambda: _outer_tin("copies"),
}
# which scenes must carry a bad-quad bitmap (the others are height fields)
BAD_MAP = {"folded sheet", "140x150 rotated 80 deg about x", "outer TIN", "outer TIN + 64 tiny triangles with one key",
           "outer TIN + 40 copies of one triangle"}


def _host_blob(hip, s, vert_grid=None):
    """Build the scene and copy its blob to the host."""
    import torch  # noqa: F401
    from horayzon_amd import dist
    nvs = 0 if s["vs"] is None else s["vs"].size // 3
    nts = 0 if s["ts"] is None else s["ts"].size // 3
    sc = hip.Scene.create(s["vert_grid"] if vert_grid is None else vert_grid, s["d0"], s["d1"], vert_simp=s["vs"],
                          num_vert_simp=nvs, tri_ind_simp=s["ts"], num_tri_simp=nts)
    try:
        p, n = sc.blob()
        blob = dist.device_bytes_or_copy(p, n, 0, owner=sc)[0].cpu().numpy().copy()
        assert blob.size == n
    finally:
        sc.close()
    return blob


def _show(findings):
    return "\n".join("%s[%d]: %s" % f for f in findings[:12])


@pytest.mark.parametrize("name", list(SCENES))
def test_device_blob_is_valid(hip, name):
    s = SCENES[name]()
    blob = _host_blob(hip, s)
    stats = {}
    findings = bvh_check.check(blob, s["vert_grid"], s["d0"], s["d1"], s["vs"], s["ts"], stats=stats)
    flags = bvh_check.decode(blob)["hdr"]["flags"]
    print(json.dumps(dict(scene=name, flags=flags, **stats)))
    if findings:
        print(_show(findings))
    assert findings == [], "%d findings, the first:\n%s" % (len(findings), _show(findings))
    assert flags == (bvh_check.HZ_BLOB_BAD_MAP if name in BAD_MAP else bvh_check.HZ_BLOB_HEIGHT_FIELD)


def _first_differences(a, b):
    h = bvh_check.decode(a)["hdr"]
    d = np.flatnonzero(a != b) if a.size == b.size else np.zeros(0, int)
    return "%d bytes differ, the first at %s (regions: verts %d, nodes %d, prims %d, anc %d, end %d)" % (
        d.size, d[:8].tolist(), h["off_verts"], h["off_nodes"], h["off_prims"], h["off_anc"], h["total_bytes"])


def test_build_is_deterministic(hip):
    """Two builds of one scene give the same bytes, and so does a build from a device-resident vert_grid."""
    import torch
    g, s = _rough(65, 65, 22)
    a, b = _host_blob(hip, s), _host_blob(hip, s)
    assert a.size == b.size and np.array_equal(a, b), _first_differences(a, b)
    x, y = np.meshgrid(g["x"], g["y"])
    dev = hip.auxiliary.rearrange_pad_buffer(*(torch.from_numpy(np.ascontiguousarray(t, np.float32)).to("cuda:0") for t in (x, y, g["z"])))
    assert dev.is_cuda
    c = _host_blob(hip, s, vert_grid=dev)
    assert a.size == c.size and np.array_equal(a, c), _first_differences(a, c)


def test_checker_understands_the_real_format(hip):
    """The mutation list of tests/test_bvh_check.py on a host copy of the real 65 x 65 blob."""
    _, s = _rough(65, 65, 22)
    blob = _host_blob(hip, s)
    assert bvh_check.check(blob, s["vert_grid"], 65, 65) == []
    muts = bvh_check.mutations(blob)
    assert len(muts) == 14
    for name, kinds, bad in muts:
        findings = bvh_check.check(bad, s["vert_grid"], 65, 65)
        got = {f.kind for f in findings}
        print(name, sorted(got))
        assert "internal" not in got, _show(findings)
        assert got & set(kinds), "%s: expected %s, got\n%s" % (name, kinds, _show(findings))


def test_checker_understands_the_real_bitmap(hip):
    """Defects of the bad-quad bitmap and of its header fields, on host copies of real blobs: a scene whose bitmap has
    marked and unmarked cells, and the cell under the middle of a TIN triangle."""
    s = _rotated("x", 80.0)
    blob = _host_blob(hip, s)
    muts = bvh_check.badmap_mutations(blob)
    assert len(muts) == 6
    for name, kinds, bad in muts:
        got = {f.kind for f in bvh_check.check(bad, s["vert_grid"], 140, 150)}
        print(name, sorted(got))
        assert "internal" not in got and got & set(kinds), (name, got)
    s = _outer_tin("ring")
    blob = _host_blob(hip, s)
    h = bvh_check.decode(blob)["hdr"]
    tri = s["vs"].reshape(-1, 3)[s["ts"].reshape(-1, 3)[0]].astype(np.float64)
    cx, cy = tri[:, 0].mean(), tri[:, 1].mean()
    i = int(bvh_check.bad_cell(np.float32(cx), h["bad_x0"], h["bad_sx"], h["bad_nb"]))
    j = int(bvh_check.bad_cell(np.float32(cy), h["bad_y0"], h["bad_sy"], h["bad_nb"]))
    cell = j * h["bad_nb"] + i
    assert blob[h["off_bad"] + cell // 8] & (1 << (cell % 8))
    blob[h["off_bad"] + cell // 8] &= np.uint8(~(1 << (cell % 8)) & 0xFF)
    got = {f.kind for f in bvh_check.check(blob, s["vert_grid"], 140, 150, s["vs"], s["ts"])}
    assert got == {"badmap"}, got
