"""Structural checker for the scene blob that hz_scene.hip builds on the device (NumPy only, no GPU work).

`decode` reads a host copy of the blob as hz_common.h describes it; `check` holds it against the guarantees that
hz_common.h and hz_scene.hip state -- exactly: every comparison is either a float32 replication of the build's own
arithmetic (the library is compiled with -ffp-contract=off, so NumPy's float32 operations round as the kernels do) or a
float64 evaluation of operands that are exact in float64.  There is no tolerance anywhere.

Finding kinds ("Blob invariants"):
  header    BlobHeader fields, region offsets, the vertex copy, scene bounds, centre and pad      (scene_build, "1. bounds")
  topology  links, block ownership, dead nodes, unused leaf slots, breadth-first numbering, height
            (k_bfs_need / k_bfs_emit / k_fill_dead_nodes)
  prims     every DEM quad / TIN triangle in exactly one present leaf slot, bit for bit           (write_prim)
  box       X(q_lo) <= lo - m and X(q_hi) >= hi + m for every present slot at every level; wrapper nodes
            (k_leaf_boxes, k_refit_pass, axis_try / axis_lo / axis_hi, k_bfs_emit)
  tight     codes are the closest the frame allows; empty halves carry the empty pair             (axis_lo / axis_hi / axis_pair)
  anc       hit-cache ancestors                                                                   (k_anc_bfs)
  badmap    height-field flag, n_flipped and the bad-quad bitmap                                  (tri_orient_xy, k_mark_bad)

`build_reference` / `mutations` exist for the tests only: a plain-Python builder of valid blobs (DEM quads only) so that
the checker is itself tested where there is no GPU, and the list of defects every test run injects into a host copy (`mutations`, and `badmap_mutations` for blobs with a bitmap).
"""
from collections import namedtuple

import numpy as np

HZ_BLOB_MAGIC = 0x485A4C42
HZ_BLOB_VERSION = 10
HZ_MAX_STACK = 40            # hz_internal.h
HZ_MAX_TOP_NODES = 2047      # hz_internal.h
HZ_ANC_LEVELS = 4            # hz_internal.h
HZ_BLOB_HEIGHT_FIELD = 1
HZ_BLOB_BAD_MAP = 2
HZ_BAD_MAX_SPAN = 512        # hz_scene.hip

HDR = np.dtype([("magic", "<u4"), ("version", "<u4"), ("d0", "<i4"), ("d1", "<i4"), ("n_quads", "<i4"),
                ("n_tin", "<i4"), ("n_prims", "<i4"), ("n_nodes", "<i4"), ("height", "<i4"), ("n_top", "<i4"),
                ("center", "<f4", 3), ("pad", "<f4"), ("lo", "<f4", 3), ("hi", "<f4", 3), ("reserved0", "<u4", 2),
                ("off_verts", "<u8"), ("off_nodes", "<u8"), ("off_prims", "<u8"), ("total_bytes", "<u8"),
                ("off_anc", "<u8"), ("anc_levels", "<i4"), ("n_prim_slots", "<i4"), ("flags", "<u4"),
                ("n_flipped", "<u4"), ("off_bad", "<u8"), ("bad_nb", "<i4"), ("bad_x0", "<f4"), ("bad_y0", "<f4"),
                ("bad_sx", "<f4"), ("bad_sy", "<f4"), ("reserved", "u1", 84)])
assert HDR.itemsize == 256
# q: qx = (lo, hi) of column half 0, of column half 1; qy the same per row half; qz = (lo, hi) of slots 0..3
NODE = np.dtype([("org", "<f4", 3), ("first", "<i4"), ("q", "u1", 16)])
assert NODE.itemsize == 32
PRIM_BYTES = 48

Finding = namedtuple("Finding", "kind index message")

_F32 = np.float32
_FLT_EPSILON = float(np.finfo(np.float32).eps)
_FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def _align(x, a=256):
    return (int(x) + a - 1) // a * a


def _dead_node():
    d = np.zeros(1, NODE)
    d["org"] = np.array([127, 0, 127], np.uint32).view(np.float32)
    d["first"] = np.int32(-2 ** 31)
    d["q"] = np.tile(np.array([255, 0], np.uint8), 8)
    return d


DEAD_BYTES = _dead_node().tobytes()


def _as_u8(blob):
    if isinstance(blob, np.ndarray):
        return np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    return np.frombuffer(bytes(blob), np.uint8)


def decode(blob_bytes):
    """Header fields (dict), vertices f32[d0*d1, 3], nodes (NODE records), prims u32[slots, 12] (raw words; view as
    float32 for coordinates), anc i32[slots] and the bad-quad bitmap words (or None) of a host copy of the blob.
    Raises ValueError where a region does not fit into the bytes given."""
    raw = _as_u8(blob_bytes)
    if raw.size < 256:
        raise ValueError("blob shorter than its header (%d bytes)" % raw.size)
    h = raw[:256].view(HDR)[0]
    hdr = {k: (h[k].copy() if h[k].ndim else h[k].item()) for k in HDR.names if not k.startswith("reserved")}
    d0, d1, n_nodes, slots = hdr["d0"], hdr["d1"], hdr["n_nodes"], hdr["n_prim_slots"]
    if d0 < 2 or d1 < 2 or d0 > 32767 or d1 > 32767 or n_nodes < 0 or slots < 0:
        raise ValueError("header sizes out of range (d0 %d, d1 %d, n_nodes %d, n_prim_slots %d)" % (d0, d1, n_nodes, slots))

    def region(off, nbytes, what):
        if off % 4 or off < 256 or off + nbytes > raw.size:
            raise ValueError("%s region [%d, %d) does not fit the %d blob bytes" % (what, off, off + nbytes, raw.size))
        return raw[off:off + nbytes]

    out = {"hdr": hdr, "nbytes": int(raw.size)}
    out["verts"] = region(hdr["off_verts"], 12 * d0 * d1, "vertex").view("<f4").reshape(-1, 3)
    out["nodes"] = region(hdr["off_nodes"], 32 * n_nodes, "node").view(NODE)
    out["prims"] = region(hdr["off_prims"], PRIM_BYTES * slots, "prim").view("<u4").reshape(-1, 12)
    out["anc"] = region(hdr["off_anc"], 4 * slots, "anc").view("<i4")
    out["bad"] = None
    if hdr["flags"] & HZ_BLOB_BAD_MAP:
        nb = hdr["bad_nb"]
        if nb < 1 or nb > 2048 or nb % 8:
            raise ValueError("bad_nb %d out of range" % nb)
        out["bad"] = region(hdr["off_bad"], nb * nb // 8, "bad map").view("<u4")
    return out


# ----------------------------------------------------------------------------------------------------------------
# float32 replications of the build's arithmetic
# ----------------------------------------------------------------------------------------------------------------
def scene_bounds(verts, vert_simp=None):
    """(lo, hi, center, pad) as scene_build computes them ("1. bounds")."""
    pts = verts.reshape(-1, 3)
    if vert_simp is not None:
        pts = np.concatenate([pts, vert_simp.reshape(-1, 3)], axis=0)
    lo, hi = pts.min(axis=0).astype(_F32), pts.max(axis=0).astype(_F32)
    center = _F32(0.5) * lo + _F32(0.5) * hi
    maxabs = float(max(np.abs(lo).max(), np.abs(hi).max()))
    diag2 = 0.0
    for k in range(3):
        diag2 += (float(hi[k]) - float(lo[k])) * (float(hi[k]) - float(lo[k]))
    pad = _F32(1.0e-6 * np.sqrt(diag2) + 4.0 * _FLT_EPSILON * maxabs) + _FLT_MIN
    return lo, hi, center, _F32(pad)


def quad_corners(verts, d0, d1):
    """a, b, c, d of every DEM quad in primitive order p = i * (d1 - 1) + j (prim_vertices)."""
    v = verts.reshape(d0, d1, 3)
    return (v[:-1, :-1].reshape(-1, 3), v[:-1, 1:].reshape(-1, 3), v[1:, :-1].reshape(-1, 3), v[1:, 1:].reshape(-1, 3))


def tri_orient_xy(p0, p1, p2):
    ux, uy = p1[..., 0] - p0[..., 0], p1[..., 1] - p0[..., 1]
    vx, vy = p2[..., 0] - p0[..., 0], p2[..., 1] - p0[..., 1]
    m0, m1 = ux * vy, uy * vx
    nz = m0 - m1
    ok = np.abs(nz) > _F32(1.0e-5) * (np.abs(m0) + np.abs(m1))
    return np.where(ok, np.where(nz > 0, 1, -1), 0)


def bad_cell(v, v0, s, nb):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((v - _F32(v0)) * _F32(s))
    return np.clip(np.nan_to_num(c, nan=0.0, posinf=2.0 ** 40, neginf=-2.0 ** 40).astype(np.int64), 0, nb - 1)


def _leaf_boxes(prims_u32, center, pad):
    """k_leaf_boxes on the records themselves (a TIN record is read as a, b, c, c)."""
    p = prims_u32.view("<f4").reshape(-1, 4, 3)
    tin = np.isnan(p[:, 3, 0])
    d = np.where(tin[:, None], p[:, 2], p[:, 3])
    with np.errstate(invalid="ignore", over="ignore"):
        mn = np.minimum(np.minimum(p[:, 0], p[:, 1]), np.minimum(p[:, 2], d))
        mx = np.maximum(np.maximum(p[:, 0], p[:, 1]), np.maximum(p[:, 2], d))
        lo = (mn - center[None, :]) - pad
        hi = (mx - center[None, :]) + pad
    return lo.astype(_F32), hi.astype(_F32)


def _steps(org):
    """(x / y step, z step) hidden in the low 9 mantissa bits of org[0] and org[2], as float64 [n, 3] per axis."""
    b = np.ascontiguousarray(org).view("<u4").reshape(-1, 3)
    sxy = ((b[:, 0] & np.uint32(0x1FF)) << np.uint32(23)).view("<f4").astype(np.float64)
    sz = ((b[:, 2] & np.uint32(0x1FF)) << np.uint32(23)).view("<f4").astype(np.float64)
    return np.stack([sxy, sxy, sz], axis=1)


# slot k uses x pair k & 1, y pair k >> 1, z pair k: byte positions of (lo, hi) in NODE.q per slot and axis
_QLO = np.array([[0 + 2 * (k & 1), 4 + 2 * (k >> 1), 8 + 2 * k] for k in range(4)])
_QHI = _QLO + 1


class _Out:
    def __init__(self, cap=25):
        self.items, self.count, self.cap = [], {}, cap

    def add(self, kind, index, msg):
        n = self.count.get(kind, 0)
        self.count[kind] = n + 1
        if n < self.cap:
            self.items.append(Finding(kind, int(index), msg))

    def each(self, kind, indices, fmt, cols=()):
        indices = np.asarray(indices).reshape(-1)
        for r in range(indices.size):
            if self.count.get(kind, 0) >= self.cap:
                self.count[kind] += indices.size - r
                return
            self.add(kind, indices[r], fmt % tuple(np.asarray(c).reshape(-1)[r] for c in cols) if cols else fmt)


def check(blob, vert_grid, d0, d1, vert_simp=None, tri_ind_simp=None, stats=None):
    """Findings (kind, node or leaf index, message) of a host copy of a scene blob built from these inputs; [] = valid.
    `stats`, a dict, receives n_nodes, leaf_fill, height and step_ratio (the largest 255 * step / node extent per axis:
    reported, never asserted)."""
    out = _Out()
    try:
        with np.errstate(all="ignore"):          # garbage decodes to NaN / inf; every comparison below is written for them
            _check(out, blob, vert_grid, int(d0), int(d1), vert_simp, tri_ind_simp, stats if stats is not None else {})
    except Exception as e:      # a checker defect, never a property of the blob: reported under a kind of its own
        out.add("internal", -1, "checker raised %s: %s" % (type(e).__name__, e))
    return out.items


def _check(out, blob, vert_grid, d0, d1, vert_simp, tri_ind_simp, stats):
    try:
        dec = decode(blob)
    except ValueError as e:
        out.add("header", -1, str(e))
        return
    h, verts, nodes, prims, anc = dec["hdr"], dec["verts"], dec["nodes"], dec["prims"], dec["anc"]
    vg = np.ascontiguousarray(np.asarray(vert_grid), np.float32).reshape(-1)
    vs = ts = None
    if vert_simp is not None and tri_ind_simp is not None:
        vs = np.ascontiguousarray(np.asarray(vert_simp), np.float32).reshape(-1)
        ts = np.ascontiguousarray(np.asarray(tri_ind_simp), np.int32).reshape(-1)
        vs, ts = vs[:vs.size // 3 * 3].reshape(-1, 3), ts[:ts.size // 3 * 3].reshape(-1, 3)
        if vs.shape[0] < 3 or ts.shape[0] < 1:
            vs = ts = None
    n_tin = 0 if ts is None else ts.shape[0]
    n_quads = (d0 - 1) * (d1 - 1)
    N, S = h["n_nodes"], h["n_prim_slots"]

    # ---- header ---------------------------------------------------------------------------------------------------
    def want(name, value, got=None):
        got = h[name] if got is None else got
        if got != value:
            out.add("header", -1, "%s is %r, expected %r" % (name, got, value))

    want("magic", HZ_BLOB_MAGIC)
    want("version", HZ_BLOB_VERSION)
    want("d0", d0)
    want("d1", d1)
    if h["d0"] != d0 or h["d1"] != d1 or vg.size < 3 * d0 * d1:
        out.add("header", -1, "grid dimensions do not match the inputs: nothing else can be checked")
        return
    want("n_quads", n_quads)
    want("n_tin", n_tin)
    want("n_prims", n_quads + n_tin)
    grid = vg[:3 * d0 * d1].reshape(-1, 3)
    diff = np.flatnonzero(verts.view("<u4").reshape(-1) != grid.view("<u4").reshape(-1))
    out.each("header", diff, "vertex word differs from vert_grid")
    lo, hi, center, pad = scene_bounds(grid, vs)
    for k in range(3):
        want("lo[%d]" % k, float(lo[k]), float(h["lo"][k]))
        want("hi[%d]" % k, float(hi[k]), float(h["hi"][k]))
        want("center[%d]" % k, float(center[k]), float(h["center"][k]))
    want("pad", float(pad))
    if N % 4 or N < 4:
        out.add("header", -1, "n_nodes %d is not a positive multiple of 4" % N)
    if S % 4:
        out.add("header", -1, "n_prim_slots %d is no multiple of 4" % S)
    want("n_top", min(N, HZ_MAX_TOP_NODES))
    want("anc_levels", HZ_ANC_LEVELS)
    # orientation census (k_leaf_boxes) decides whether the blob carries a bitmap region
    qa, qb, qc, qd = quad_corners(grid, d0, d1)
    o0, o1 = tri_orient_xy(qa, qb, qc), tri_orient_xy(qb, qd, qc)
    n_pos = int((o0 > 0).sum() + (o1 > 0).sum())
    n_neg = int((o0 < 0).sum() + (o1 < 0).sum())
    n_deg = int((o0 == 0).sum() + (o1 == 0).sum())
    majority = 1 if n_pos >= n_neg else -1
    n_flipped = min(n_pos, n_neg) + n_deg
    height_field = n_flipped == 0 and n_quads > 0 and n_tin == 0
    want("off_verts", 256)
    off_nodes = _align(256 + 12 * d0 * d1)
    off_prims = _align(off_nodes + 32 * N)
    off_anc = _align(off_prims + PRIM_BYTES * S)
    total = _align(off_anc + 4 * S)
    nb = 8
    while nb < 2048 and 2 * nb < max(d0, d1):
        nb *= 2
    off_bad = 0
    if not height_field:
        off_bad = total
        total = _align(off_bad + nb * nb // 8)
    want("off_nodes", off_nodes)
    want("off_prims", off_prims)
    want("off_anc", off_anc)
    want("total_bytes", total)
    if dec["nbytes"] != total:
        out.add("header", -1, "the blob has %d bytes, its layout needs %d" % (dec["nbytes"], total))
    # the bytes between the regions are zero: two builds of one scene give the same bytes
    raw = _as_u8(blob)
    ends = [(256 + 12 * d0 * d1, off_nodes), (off_nodes + 32 * N, off_prims), (off_prims + PRIM_BYTES * S, off_anc)]
    ends.append((off_anc + 4 * S, off_bad if off_bad else total))
    if off_bad:
        ends.append((off_bad + nb * nb // 8, total))
    for a, b in ends:
        if 0 <= a <= b <= raw.size and raw[a:b].any():
            out.add("header", a + int(np.flatnonzero(raw[a:b])[0]), "padding bytes [%d, %d) between two regions are not zero" % (a, b))
    if N % 4 or S % 4 or N < 4:
        return

    # ---- topology: level by level from the root ------------------------------------------------------------------------
    first = nodes["first"].astype(np.int64)
    q = nodes["q"]
    present = ~((q[:, 8::2] == 255) & (q[:, 9::2] == 0))                    # [N, 4]
    node_bytes = np.ascontiguousarray(nodes).view(np.uint8).reshape(N, 32)
    dead = (node_bytes == np.frombuffer(DEAD_BYTES, np.uint8)[None, :]).all(axis=1)
    depth = np.full(N, -1, np.int64)
    parent = np.full(N, -1, np.int64)
    pslot = np.full(N, -1, np.int64)
    link_ok = np.zeros(N, bool)                  # the node's `first` addresses a block that it owns
    nb_owner = np.zeros(N // 4, np.int64)
    lb_owner = np.zeros(S // 4, np.int64)
    lb_parent = np.full(S // 4, -1, np.int64)
    if dead[0]:
        out.add("topology", 0, "node 0 is not the root but a dead node")
    for k in (1, 2, 3):
        if not dead[k]:
            out.add("topology", k, "node %d of the root's block is not the dead pattern of k_fill_dead_nodes" % k)
    frontier = np.array([0], np.int64)
    depth[0] = 0
    level = 0
    while frontier.size:
        if level >= HZ_MAX_STACK:
            out.add("topology", frontier[0], "links are deeper than HZ_MAX_STACK = %d levels" % HZ_MAX_STACK)
            break
        f = first[frontier]
        is_leaf = f < 0
        idx = np.where(is_leaf, f & 0x7FFFFFFF, f)
        limit = np.where(is_leaf, S, N)
        bad = (idx % 4 != 0) | (idx + 3 >= limit)
        out.each("topology", frontier[bad], "first = %#x is not a 4-aligned block in range", (f[bad] & 0xFFFFFFFF,))
        cyc = ~bad & ~is_leaf & (idx == 0)
        out.each("topology", frontier[cyc], "first = 0 links back to the root's block (a cycle)")
        ok = ~bad & ~cyc
        sel = ok & is_leaf
        np.add.at(lb_owner, idx[sel] // 4, 1)
        lb_parent[idx[sel] // 4] = frontier[sel]
        link_ok[frontier[sel]] = True
        sel = np.flatnonzero(ok & ~is_leaf)
        blocks = idx[sel] // 4
        fresh = nb_owner[blocks] == 0
        np.add.at(nb_owner, blocks, 1)
        _, firsts = np.unique(blocks, return_index=True)
        keep = np.zeros(sel.size, bool)
        keep[firsts] = True
        sel = sel[keep & fresh]                  # a block is descended into once, by its first owner: the walk ends
        own = frontier[sel]
        link_ok[own] = True
        child = idx[sel][:, None] + np.arange(4)[None, :]
        pres = present[own]
        cdead = dead[child]
        seen = depth[child] >= 0
        out.each("topology", child[pres & cdead], "present slot %d of node %d holds a dead node",
                 (np.broadcast_to(np.arange(4), child.shape)[pres & cdead], np.broadcast_to(own[:, None], child.shape)[pres & cdead]))
        out.each("topology", child[~pres & ~cdead], "absent slot of node %d is not the dead pattern",
                 (np.broadcast_to(own[:, None], child.shape)[~pres & ~cdead],))
        out.each("topology", child[pres & seen], "node is reached a second time")
        go = pres & ~cdead & ~seen
        nxt = child[go]
        depth[nxt] = level + 1
        parent[nxt] = np.broadcast_to(own[:, None], child.shape)[go]
        pslot[nxt] = np.broadcast_to(np.arange(4), child.shape)[go]
        frontier = nxt
        level += 1
    live = depth >= 0
    out.each("topology", np.flatnonzero(~live & ~dead), "a node that is no dead node is not reached from the root")
    blk = np.arange(1, N // 4)
    out.each("topology", 4 * blk[nb_owner[1:] == 0], "node block is owned by no node")
    out.each("topology", 4 * blk[nb_owner[1:] > 1], "node block is owned by %d nodes", (nb_owner[1:][nb_owner[1:] > 1],))
    if nb_owner[0]:
        out.add("topology", 0, "the root's block is owned by a node")
    out.each("topology", 4 * np.flatnonzero(lb_owner == 0), "leaf block is owned by no node")
    out.each("topology", 4 * np.flatnonzero(lb_owner > 1), "leaf block is owned by %d nodes", (lb_owner[lb_owner > 1],))
    n_present = present.sum(axis=1)
    out.each("topology", np.flatnonzero(live & (n_present == 0)), "live node without a present slot")
    wrapper = live & (n_present == 1) & (np.arange(N) > 0)
    out.each("topology", np.flatnonzero(wrapper & ~(present[:, 0] & (first < 0))),
             "single-child node is not a wrapper (slot 0, one leaf block)")
    live_idx = np.flatnonzero(live)
    drop = np.flatnonzero(np.diff(depth[live_idx]) < 0)
    out.each("topology", live_idx[drop + 1], "numbering is not breadth first: depth %d follows depth %d",
             (depth[live_idx[drop + 1]], depth[live_idx[drop]]))
    max_depth = int(depth.max())
    if h["height"] != 1 + max_depth:
        out.add("topology", -1, "height is %d, the deepest node has depth %d" % (h["height"], max_depth))
    if h["height"] > HZ_MAX_STACK:
        out.add("topology", -1, "height %d exceeds HZ_MAX_STACK" % h["height"])
    # leaf slots: present <-> a record, absent <-> 48 zero bytes
    owned = np.flatnonzero((lb_owner == 1) & (lb_parent >= 0))
    slot_present = np.zeros(S, bool)
    slot_present.reshape(-1, 4)[owned] = present[lb_parent[owned]]
    slot_owned = np.zeros(S, bool)
    slot_owned.reshape(-1, 4)[owned] = True
    zero = ~prims.any(axis=1)
    out.each("topology", np.flatnonzero(slot_owned & slot_present & zero), "present leaf slot holds no record (48 zero bytes)")
    out.each("topology", np.flatnonzero(slot_owned & ~slot_present & ~zero), "absent leaf slot is not 48 zero bytes")

    # ---- prims: the multiset of records in present slots == the multiset of the scene's primitives ----------------------
    def canon(rec):             # a TIN record is a, b, c and a NaN in d.x; d.y, d.z are not part of the contract
        rec = rec.copy()
        tin = np.isnan(rec.view("<f4")[:, 9])
        rec[tin, 9] = 0x7FC00000
        rec[tin, 10:] = 0
        return rec

    exp = np.concatenate([qa, qb, qc, qd], axis=1).view("<u4")
    if n_tin:
        if ts.min() < 0 or ts.max() >= vs.shape[0]:
            raise ValueError("tri_ind_simp addresses vertices that vert_simp does not have")
        t = np.concatenate([vs[ts[:, 0]], vs[ts[:, 1]], vs[ts[:, 2]], np.full((n_tin, 3), np.nan, _F32)], axis=1)
        exp = np.concatenate([exp, canon(np.ascontiguousarray(t).view("<u4"))], axis=0)
    act_slots = np.flatnonzero(slot_present & ~zero)
    act = canon(prims[act_slots])
    _, inv = np.unique(np.concatenate([exp, act], axis=0), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    n_kinds = int(inv.max()) + 1 if inv.size else 0
    c_exp = np.bincount(inv[:exp.shape[0]], minlength=n_kinds)
    c_act = np.bincount(inv[exp.shape[0]:], minlength=n_kinds)
    missing = np.flatnonzero(c_exp[inv[:exp.shape[0]]] > c_act[inv[:exp.shape[0]]])
    out.each("prims", missing, "primitive occurs %d times among the leaf records, the scene has it %d times",
             (c_act[inv[:exp.shape[0]]][missing], c_exp[inv[:exp.shape[0]]][missing]))
    ia = inv[exp.shape[0]:]
    extra = np.flatnonzero(c_act[ia] > c_exp[ia])
    out.each("prims", act_slots[extra], "leaf record occurs %d times, the scene has that primitive %d times",
             (c_act[ia][extra], c_exp[ia][extra]))

    # ---- box: leaf boxes, float32 unions bottom up, containment in float64 -------------------------------------------
    bc, bpad = h["center"].astype(_F32), _F32(h["pad"])          # (both already held to the inputs above)
    leaf_lo, leaf_hi = _leaf_boxes(prims, bc, bpad)
    use = slot_present & ~zero
    leaf_lo[~use] = np.inf
    leaf_hi[~use] = -np.inf
    slot_lo = np.full((N, 4, 3), np.inf, _F32)
    slot_hi = np.full((N, 4, 3), -np.inf, _F32)
    node_lo = np.full((N, 3), np.inf, _F32)
    node_hi = np.full((N, 3), -np.inf, _F32)
    for lev in range(max_depth, -1, -1):
        at = np.flatnonzero((depth == lev) & link_ok)
        lf = at[first[at] < 0]
        base = (first[lf] & 0x7FFFFFFF)[:, None] + np.arange(4)[None, :]
        slot_lo[lf], slot_hi[lf] = leaf_lo[base], leaf_hi[base]
        nd = at[first[at] >= 0]
        base = first[nd][:, None] + np.arange(4)[None, :]
        ok = (present[nd] & (parent[base] == nd[:, None]))[:, :, None]
        slot_lo[nd] = np.where(ok, node_lo[base], np.inf)
        slot_hi[nd] = np.where(ok, node_hi[base], -np.inf)
        node_lo[at], node_hi[at] = slot_lo[at].min(axis=1), slot_hi[at].max(axis=1)
    org = nodes["org"].astype(np.float64)
    step = _steps(nodes["org"])                                    # [N, 3]
    m = step / 4096.0
    qlo = q[:, _QLO].astype(np.float64)                            # [N, 4, 3]
    qhi = q[:, _QHI].astype(np.float64)

    def plane(code):
        return org[:, None, :] + (1024.0 + code) * step[:, None, :]

    have = (present & live[:, None])[:, :, None] & np.isfinite(slot_lo) & np.isfinite(slot_hi)
    want_lo = slot_lo.astype(np.float64) - m[:, None, :]
    want_hi = slot_hi.astype(np.float64) + m[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        bad_lo = have & ~(plane(qlo) <= want_lo)
        bad_hi = have & ~(plane(qhi) >= want_hi)
    for bad_, name, code, wanted in ((bad_lo, "lower", qlo, want_lo), (bad_hi, "upper", qhi, want_hi)):
        n_, k_, a_ = np.nonzero(bad_)
        out.each("box", n_, "slot %d axis %d: %s plane of code %d at %.17g does not cover %.17g",
                 (k_, a_, np.full(n_.size, name), code[bad_].astype(np.int64), plane(code)[bad_], wanted[bad_]))
    # wrapper nodes: the parent's origins, that slot's three pairs in slot 0, everything else empty
    w = np.flatnonzero(wrapper & present[:, 0] & (first < 0) & (parent >= 0))
    pw, kw_ = parent[w], pslot[w]
    org_bits = np.ascontiguousarray(nodes["org"]).view("<u4").reshape(N, 3)
    expq = np.tile(np.array([255, 0], np.uint8), (w.size, 8))
    for a in range(3):
        expq[:, 4 * a] = q[pw, _QLO[kw_, a]]
        expq[:, 4 * a + 1] = q[pw, _QHI[kw_, a]]
    wrong = (org_bits[w] != org_bits[pw]).any(axis=1) | (q[w] != expq).any(axis=1)
    out.each("box", w[wrong], "wrapper node does not carry slot %d of its parent %d", (kw_[wrong], pw[wrong]))

    # ---- tight: per pair (a half's x / y pair over the present slots of that half, a slot's z pair) ---------------------
    regular = live & link_ok & ~wrapper
    inf32 = _F32(np.inf)
    pairs = []                                                     # (axis, byte of lo code, range lo [N], range hi [N], any [N])
    for hlf in range(2):
        for a, ks in ((0, [k for k in range(4) if (k & 1) == hlf]), (1, [k for k in range(4) if (k >> 1) == hlf])):
            pr = present[:, ks]
            l_ = np.where(pr, slot_lo[:, ks, a], inf32).min(axis=1)
            h_ = np.where(pr, slot_hi[:, ks, a], -inf32).max(axis=1)
            pairs.append((a, 4 * a + 2 * hlf, l_, h_, pr.any(axis=1)))
    for k in range(4):
        pairs.append((2, 8 + 2 * k, slot_lo[:, k, 2], slot_hi[:, k, 2], present[:, k]))
    for a, byte, l_, h_, anyp in pairs:
        cl, ch = q[:, byte].astype(np.float64), q[:, byte + 1].astype(np.float64)
        fin = regular & anyp & np.isfinite(l_) & np.isfinite(h_)
        wl, wh = l_.astype(np.float64) - m[:, a], h_.astype(np.float64) + m[:, a]
        with np.errstate(invalid="ignore", over="ignore"):
            loose_lo = fin & (cl < 255) & ~(org[:, a] + (1024.0 + cl + 1.0) * step[:, a] > wl)
            loose_hi = fin & (ch > 0) & ~(org[:, a] + (1024.0 + ch - 1.0) * step[:, a] < wh)
        out.each("tight", np.flatnonzero(loose_lo), "axis %d pair at byte %d: lower code %d is not maximal",
                 (np.full(N, a)[loose_lo], np.full(N, byte)[loose_lo], cl[loose_lo].astype(np.int64)))
        out.each("tight", np.flatnonzero(loose_hi), "axis %d pair at byte %d: upper code %d is not minimal",
                 (np.full(N, a)[loose_hi], np.full(N, byte)[loose_hi], ch[loose_hi].astype(np.int64)))
        if a < 2:
            stray = regular & ~anyp & ~((cl == 255) & (ch == 0))
            out.each("tight", np.flatnonzero(stray), "axis %d half without a present slot has the pair (%d, %d)",
                     (np.full(N, a)[stray], cl[stray].astype(np.int64), ch[stray].astype(np.int64)))
    ratio = [0.0, 0.0, 0.0]
    reg = np.flatnonzero(regular & np.isfinite(node_lo).all(axis=1) & np.isfinite(node_hi).all(axis=1))
    if reg.size:
        ext = node_hi[reg].astype(np.float64) - node_lo[reg].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = [float(x) for x in np.nanmax(np.where(ext > 0, 255.0 * step[reg] / ext, np.nan), axis=0)]
    stats.update(n_nodes=int(N), n_live=int(live.sum()), leaf_fill=float(use.sum()) / max(S, 1), height=int(h["height"]),
                 step_ratio=ratio)

    # ---- anc -----------------------------------------------------------------------------------------------------
    n_ = lb_parent[owned].copy()
    for _ in range(max(1, h["anc_levels"]) - 1):
        p_ = parent[n_]
        n_ = np.where(p_ >= 0, p_, n_)
    got = anc.reshape(-1, 4)[owned]
    wrong = got != n_[:, None]
    r_, c_ = np.nonzero(wrong)
    out.each("anc", 4 * owned[r_] + c_, "anc is %d, the node %d levels above the leaf is %d",
             (got[wrong], np.full(r_.size, max(1, h["anc_levels"])), n_[r_]))

    # ---- badmap --------------------------------------------------------------------------------------------------
    _check_badmap(out, dec, grid, d0, d1, vs, ts, lo, hi, nb, off_bad, majority, n_flipped, height_field, o0, o1)


def _mark_rects(nb, i0, i1, j0, j1):
    """OR of the cell boxes [i0, i1] x [j0, j1] as a bool [nb (y), nb (x)] map."""
    acc = np.zeros((nb + 1, nb + 1), np.int64)
    np.add.at(acc, (j0, i0), 1)
    np.add.at(acc, (j0, i1 + 1), -1)
    np.add.at(acc, (j1 + 1, i0), -1)
    np.add.at(acc, (j1 + 1, i1 + 1), 1)
    return acc.cumsum(axis=0).cumsum(axis=1)[:nb, :nb] > 0


def _check_badmap(out, dec, grid, d0, d1, vs, ts, lo, hi, nb, off_bad, majority, n_flipped, height_field, o0, o1):
    h = dec["hdr"]
    n_tin = 0 if ts is None else ts.shape[0]
    if h["n_flipped"] != n_flipped:
        out.add("badmap", -1, "n_flipped is %d, %d triangles are minority-oriented or degenerate" % (h["n_flipped"], n_flipped))
    if height_field:
        if h["flags"] != HZ_BLOB_HEIGHT_FIELD:
            out.add("badmap", -1, "flags are %#x for a height field without a TIN" % h["flags"])
        if h["off_bad"] != 0 or h["bad_nb"] != 0:
            out.add("badmap", -1, "a height-field blob carries a bitmap (off_bad %d, bad_nb %d)" % (h["off_bad"], h["bad_nb"]))
        return
    if h["flags"] & HZ_BLOB_HEIGHT_FIELD:
        out.add("badmap", -1, "HEIGHT_FIELD is set with n_flipped = %d, n_tin = %d" % (n_flipped, n_tin))
    sx = _F32(nb) / (hi[0] - lo[0]) if hi[0] > lo[0] else _F32(0)
    sy = _F32(nb) / (hi[1] - lo[1]) if hi[1] > lo[1] else _F32(0)
    for name, value in (("bad_nb", nb), ("bad_x0", float(lo[0])), ("bad_y0", float(lo[1])), ("bad_sx", float(sx)),
                        ("bad_sy", float(sy)), ("off_bad", off_bad)):
        if h[name] != value:
            out.add("badmap", -1, "%s is %r, expected %r" % (name, h[name], value))
            return
    # footprints (k_mark_bad): bad quads, then TIN triangles
    qa, qb, qc, qd = quad_corners(grid, d0, d1)
    badq = ~((o0 == majority) & (o1 == majority))

    def cell_box(pts):        # pts [n, corners, 3]
        xl, xh, yl, yh = pts[:, :, 0].min(axis=1), pts[:, :, 0].max(axis=1), pts[:, :, 1].min(axis=1), pts[:, :, 1].max(axis=1)
        i0 = np.maximum(bad_cell(xl, lo[0], sx, nb) - 1, 0)
        i1 = np.minimum(bad_cell(xh, lo[0], sx, nb) + 1, nb - 1)
        j0 = np.maximum(bad_cell(yl, lo[1], sy, nb) - 1, 0)
        j1 = np.minimum(bad_cell(yh, lo[1], sy, nb) + 1, nb - 1)
        return i0, i1, j0, j1

    qi0, qi1, qj0, qj1 = cell_box(np.stack([qa[badq], qb[badq], qc[badq], qd[badq]], axis=1))
    overflow = bool(((qi1 - qi0 >= HZ_BAD_MAX_SPAN) | (qj1 - qj0 >= HZ_BAD_MAX_SPAN)).any())
    if n_tin:
        tri = np.stack([vs[ts[:, 0]], vs[ts[:, 1]], vs[ts[:, 2]]], axis=1)
        ti0, ti1, tj0, tj1 = cell_box(tri)
        overflow = overflow or bool(((ti1 - ti0 >= HZ_BAD_MAX_SPAN) | (tj1 - tj0 >= HZ_BAD_MAX_SPAN)).any())
    expect_map = sx > 0 and sy > 0 and not overflow
    if bool(h["flags"] & HZ_BLOB_BAD_MAP) != expect_map:
        out.add("badmap", -1, "BAD_MAP is %s, expected %s" % (bool(h["flags"] & HZ_BLOB_BAD_MAP), expect_map))
        return
    if not expect_map:
        return
    bits = np.unpackbits(dec["bad"].view(np.uint8), bitorder="little").reshape(nb, nb).astype(bool)
    quads_map = _mark_rects(nb, qi0, qi1, qj0, qj1)
    if not n_tin:
        j_, i_ = np.nonzero(bits != quads_map)
        out.each("badmap", j_ * nb + i_, "bitmap cell (x %d, y %d) is %d, the bad quads' cell boxes give %d",
                 (i_, j_, bits[j_, i_], quads_map[j_, i_]))
        return
    j_, i_ = np.nonzero(quads_map & ~bits)
    out.each("badmap", j_ * nb + i_, "bitmap cell (x %d, y %d) of a bad quad's cell box is not set", (i_, j_))
    # every cell whose rectangle meets a TIN triangle's (x, y) footprint, in float64 (separating axes: the cell's two
    # and the triangle's three); a point beyond the last cell edge belongs to the last cell, as bad_cell clamps
    t64 = tri[:, :, :2].astype(np.float64)
    ex = float(lo[0]) + np.arange(nb + 1) / float(sx)
    ey = float(lo[1]) + np.arange(nb + 1) / float(sy)
    ex[0], ey[0] = min(ex[0], t64[:, :, 0].min()), min(ey[0], t64[:, :, 1].min())
    ex[-1], ey[-1] = max(ex[-1], t64[:, :, 0].max()), max(ey[-1], t64[:, :, 1].max())
    need = np.zeros((nb, nb), bool)
    for p in t64:
        ci = np.flatnonzero((ex[1:] >= p[:, 0].min()) & (ex[:-1] <= p[:, 0].max()))
        cj = np.flatnonzero((ey[1:] >= p[:, 1].min()) & (ey[:-1] <= p[:, 1].max()))
        if not ci.size or not cj.size:
            continue
        hit = np.ones((cj.size, ci.size), bool)
        area = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
        if area != 0.0:
            sgn = 1.0 if area > 0 else -1.0
            for k in range(3):
                k1 = (k + 1) % 3
                nx, ny = sgn * (p[k1, 1] - p[k, 1]), -sgn * (p[k1, 0] - p[k, 0])       # outward normal of edge k -> k1
                # the cell corner that lies deepest on the inner side of the edge
                cx = np.where(nx > 0, ex[ci], ex[ci + 1])
                cy = np.where(ny > 0, ey[cj], ey[cj + 1])
                hit &= ~(nx * (cx[None, :] - p[k, 0]) + ny * (cy[:, None] - p[k, 1]) > 0.0)
        need[np.ix_(cj, ci)] |= hit
    j_, i_ = np.nonzero(need & ~bits)
    out.each("badmap", j_ * nb + i_, "bitmap cell (x %d, y %d) meets a TIN triangle and is not set", (i_, j_))


# ----------------------------------------------------------------------------------------------------------------
# test support: a plain-Python builder of valid blobs (DEM quads only) and the defects the tests inject
# ----------------------------------------------------------------------------------------------------------------
def _f32_bits(x):
    return int(np.array([x], "<f4").view("<u4")[0])


def _bits_f32(b):
    return np.array([b & 0xFFFFFFFF], "<u4").view("<f4")[0]


def _f32_at_most(x):
    """The largest float32 <= x (x a Python float)."""
    f = np.float32(x)
    return f if float(f) <= x else np.nextafter(f, _F32(-np.inf))


def _embed_at_most(x, e):
    """The largest float32 <= x whose low 9 mantissa bits are the biased exponent e (always a negative normal float or a
    positive normal one: a target near zero moves to the negative side)."""
    f = float(_f32_at_most(x))
    if f >= 0.0:
        b = _f32_bits(f)
        c = (b & ~0x1FF) | e
        if c > b:
            c -= 0x200
        if c >= 0x00800000:
            return _bits_f32(c)
        f = -1.0e-30
    mag = _f32_bits(f) & 0x7FFFFFFF
    c = (mag & ~0x1FF) | e
    if c < mag:
        c += 0x200
    return _bits_f32(0x80000000 | c)


def _ref_frame(nl, nh, embed):
    """Smallest power-of-two step (biased exponent) and an origin with X(0) <= nl - m and X(255) >= nh + m."""
    ext = max(float(nh) - float(nl), 1.0e-30)
    e = int(np.clip(np.floor(np.log2(ext / 255.0)) + 127 - 1, 1, 254))
    while True:
        s = 2.0 ** (e - 127)
        m = s / 4096.0
        tgt = float(nl) - m - 1024.0 * s
        o = float(_embed_at_most(tgt, e) if embed else _f32_at_most(tgt))
        if (o + 1024.0 * s <= float(nl) - m and o + 1279.0 * s >= float(nh) + m) or e >= 254:
            return e, s, o
        e += 1


def _ref_codes(o, s, lo, hi):
    m = s / 4096.0
    wl, wh = float(lo) - m, float(hi) + m
    ql = int(np.clip(np.floor((wl - o) / s) - 1024, 0, 255))
    while ql > 0 and o + (1024 + ql) * s > wl:
        ql -= 1
    while ql < 255 and o + (1025 + ql) * s <= wl:
        ql += 1
    qh = int(np.clip(np.ceil((wh - o) / s) - 1024, 0, 255))
    while qh < 255 and o + (1024 + qh) * s < wh:
        qh += 1
    while qh > 0 and o + (1023 + qh) * s >= wh:
        qh -= 1
    return ql, qh


def build_reference(vert_grid, d0, d1):
    """A valid blob for a DEM without a TIN (a height field or not), built the slow and obvious way: a recursive quadtree over the quads' grid
    index along the 2-bit Morton digits (a subtree with one quad is a leaf; levels with a single occupied quadrant are
    skipped, as the radix tree skips them), bounds quantised outward with the smallest power-of-two step that fits,
    breadth-first numbering with contiguous blocks, wrapper nodes, dead nodes and `anc`.  Not the device's bytes -- the
    device's invariants."""
    vg = np.ascontiguousarray(np.asarray(vert_grid), np.float32).reshape(-1)
    grid = vg[:3 * d0 * d1].reshape(-1, 3)
    lo, hi, center, pad = scene_bounds(grid)
    qa, qb, qc, qd = quad_corners(grid, d0, d1)
    o0, o1 = tri_orient_xy(qa, qb, qc), tri_orient_xy(qb, qd, qc)
    n_pos, n_neg = int((o0 > 0).sum() + (o1 > 0).sum()), int((o0 < 0).sum() + (o1 < 0).sum())
    majority = 1 if n_pos >= n_neg else -1
    n_flipped = min(n_pos, n_neg) + int((o0 == 0).sum() + (o1 == 0).sum())
    rec = np.concatenate([qa, qb, qc, qd], axis=1).view("<u4")
    blo, bhi = _leaf_boxes(rec, center, pad)
    ni, nj = d0 - 1, d1 - 1

    def subtree(i0, j0, size):
        """('leaf', p) | ('node', [child or None] * 4, box lo, box hi) | None for the quads in [i0, i0+size) x [j0, j0+size)."""
        if i0 >= ni or j0 >= nj:
            return None
        if size == 1:
            return ("leaf", i0 * nj + j0)
        half = size // 2
        kids = [subtree(i0 + half * (k >> 1), j0 + half * (k & 1), half) for k in range(4)]
        some = [c for c in kids if c is not None]
        if len(some) == 1:
            return some[0]
        return ("node", kids)

    size = 1
    while size < max(ni, nj):
        size *= 2
    root = subtree(0, 0, size)
    if root[0] == "leaf":
        root = ("node", [root, None, None, None])

    def box_of(t):
        if t[0] == "leaf":
            return blo[t[1]], bhi[t[1]]
        bl = [box_of(c) for c in t[1] if c is not None]
        return np.min([b[0] for b in bl], axis=0), np.max([b[1] for b in bl], axis=0)

    nodes, prims, anc_parent = [_dead_node() for _ in range(4)], [], []
    parent = {0: -1}
    level = [(0, root)]              # (node index, tree): wrapper entries are ('wrap', leaf)
    depth = 0
    while level:
        depth += 1
        nxt = []
        for self_i, t in level:
            n = nodes[self_i]
            if t[0] == "wrap":        # header written by the parent
                n["first"] = np.int32(-2 ** 31 + len(prims))
                anc_parent.append(self_i)
                prims.extend([rec[t[1]], None, None, None])
                continue
            kids = t[1]
            boxes = [box_of(c) if c is not None else None for c in kids]
            nl = np.min([b[0] for b in boxes if b is not None], axis=0)
            nh = np.max([b[1] for b in boxes if b is not None], axis=0)
            ext = max(float(nh[0]) - float(nl[0]), float(nh[1]) - float(nl[1]), 1.0e-30)
            e_xy = int(np.clip(np.floor(np.log2(ext / 255.0)) + 126, 1, 254))
            while True:                   # x and y share one step; the x origin carries its exponent
                s = 2.0 ** (e_xy - 127)
                m = s / 4096.0
                ox_ = float(_embed_at_most(float(nl[0]) - m - 1024.0 * s, e_xy))
                oy_ = float(_f32_at_most(float(nl[1]) - m - 1024.0 * s))
                if (ox_ + 1279.0 * s >= float(nh[0]) + m and oy_ + 1279.0 * s >= float(nh[1]) + m) or e_xy >= 254:
                    break
                e_xy += 1
            ez_, sz_, oz_ = _ref_frame(nl[2], nh[2], True)
            n["org"] = np.array([ox_, oy_, oz_], np.float32)
            q = np.tile(np.array([255, 0], np.uint8), 8)
            for hlf in range(2):
                for a, o_, ks in ((0, ox_, [k for k in range(4) if (k & 1) == hlf]), (1, oy_, [k for k in range(4) if (k >> 1) == hlf])):
                    bs = [boxes[k] for k in ks if boxes[k] is not None]
                    if bs:
                        q[4 * a + 2 * hlf:4 * a + 2 * hlf + 2] = _ref_codes(o_, s, min(b[0][a] for b in bs), max(b[1][a] for b in bs))
            for k in range(4):
                if boxes[k] is not None:
                    q[8 + 2 * k:10 + 2 * k] = _ref_codes(oz_, sz_, boxes[k][0][2], boxes[k][1][2])
            n["q"] = q
            if all(c is None or c[0] == "leaf" for c in kids):
                n["first"] = np.int32(-2 ** 31 + len(prims))
                anc_parent.append(self_i)
                prims.extend([rec[c[1]] if c is not None else None for c in kids])
                continue
            n["first"] = len(nodes)
            for k, c in enumerate(kids):
                new = _dead_node()
                if c is not None:
                    parent[len(nodes)] = self_i
                    if c[0] == "leaf":
                        new["org"] = n["org"][0]
                        wq = np.tile(np.array([255, 0], np.uint8), 8)
                        for a in range(3):
                            wq[4 * a], wq[4 * a + 1] = q[_QLO[k, a]], q[_QHI[k, a]]
                        new["q"] = wq
                        nxt.append((len(nodes), ("wrap", c[1])))
                    else:
                        nxt.append((len(nodes), c))
                nodes.append(new)
        level = nxt
    n_nodes, slots = len(nodes), len(prims)
    anc = []
    for p in anc_parent:
        n = p
        for _ in range(HZ_ANC_LEVELS - 1):
            if parent[n] >= 0:
                n = parent[n]
        anc.extend([n] * 4)
    hdr = np.zeros(1, HDR)
    off_nodes = _align(256 + 12 * d0 * d1)
    off_prims = _align(off_nodes + 32 * n_nodes)
    off_anc = _align(off_prims + PRIM_BYTES * slots)
    total = _align(off_anc + 4 * slots)
    extra = dict(flags=HZ_BLOB_HEIGHT_FIELD)
    bitmap = None
    if n_flipped:                     # not a height field: every bad quad marks its cell box +- 1 cell, one cell at a time
        nb = 8
        while nb < 2048 and 2 * nb < max(d0, d1):
            nb *= 2
        sx = _F32(nb) / (hi[0] - lo[0]) if hi[0] > lo[0] else _F32(0)
        sy = _F32(nb) / (hi[1] - lo[1]) if hi[1] > lo[1] else _F32(0)
        extra = dict(flags=0, bad_nb=nb, bad_x0=lo[0], bad_y0=lo[1], bad_sx=sx, bad_sy=sy, off_bad=total)
        bitmap = np.zeros(nb * nb, bool)
        ok = sx > 0 and sy > 0
        for p in np.flatnonzero(~((o0 == majority) & (o1 == majority))) if ok else []:
            xs = [float(c[p, 0]) for c in (qa, qb, qc, qd)]
            ys = [float(c[p, 1]) for c in (qa, qb, qc, qd)]
            ci = [int(bad_cell(_F32(v), lo[0], sx, nb)) for v in (min(xs), max(xs))]
            cj = [int(bad_cell(_F32(v), lo[1], sy, nb)) for v in (min(ys), max(ys))]
            i0, i1, j0, j1 = max(ci[0] - 1, 0), min(ci[1] + 1, nb - 1), max(cj[0] - 1, 0), min(cj[1] + 1, nb - 1)
            if i1 - i0 >= HZ_BAD_MAX_SPAN or j1 - j0 >= HZ_BAD_MAX_SPAN:
                ok = False
                break
            for j in range(j0, j1 + 1):
                for i in range(i0, i1 + 1):
                    bitmap[j * nb + i] = True
        if ok:
            extra["flags"] = HZ_BLOB_BAD_MAP
        total = _align(total + nb * nb // 8)
    for k, v in dict(magic=HZ_BLOB_MAGIC, version=HZ_BLOB_VERSION, d0=d0, d1=d1, n_quads=ni * nj, n_tin=0, n_prims=ni * nj,
                     n_nodes=n_nodes, height=depth, n_top=min(n_nodes, HZ_MAX_TOP_NODES), center=center, pad=pad, lo=lo,
                     hi=hi, off_verts=256, off_nodes=off_nodes, off_prims=off_prims, total_bytes=total, off_anc=off_anc,
                     anc_levels=HZ_ANC_LEVELS, n_prim_slots=slots, n_flipped=n_flipped, **extra).items():
        hdr[k] = v
    blob = np.zeros(total, np.uint8)
    blob[:256] = hdr.view(np.uint8)
    blob[256:256 + 12 * d0 * d1] = grid.view(np.uint8).reshape(-1)
    blob[off_nodes:off_nodes + 32 * n_nodes] = np.concatenate(nodes).view(np.uint8)
    pr = np.zeros((slots, 12), "<u4")
    for k, r in enumerate(prims):
        if r is not None:
            pr[k] = r
    blob[off_prims:off_prims + PRIM_BYTES * slots] = pr.view(np.uint8).reshape(-1)
    blob[off_anc:off_anc + 4 * slots] = np.array(anc, "<i4").view(np.uint8)
    if bitmap is not None and extra["flags"]:
        blob[extra["off_bad"]:extra["off_bad"] + bitmap.size // 8] = np.packbits(bitmap, bitorder="little")
    return blob


def mutations(blob):
    """[(name, kinds of which at least one must be reported, mutated host copy)] -- the defects of the issue's list,
    placed from a decode of `blob`, which must be valid and hold at least two leaf blocks.  Host memory only: a mutated
    blob is for `check`, never for a kernel."""
    src = _as_u8(blob).copy()
    dec = decode(src)
    h, nodes, prims = dec["hdr"], dec["nodes"], dec["prims"]
    N, S = h["n_nodes"], h["n_prim_slots"]
    on, op, oa = h["off_nodes"], h["off_prims"], h["off_anc"]
    q = nodes["q"]
    present = ~((q[:, 8::2] == 255) & (q[:, 9::2] == 0))
    first = nodes["first"].astype(np.int64)
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(N, 32)
    dead = (raw == np.frombuffer(DEAD_BYTES, np.uint8)[None, :]).all(axis=1)
    regular = ~dead & (present.sum(axis=1) >= 2)
    res = []

    def mutated(name, kinds, edit):
        b = src.copy()
        edit(b)
        res.append((name, kinds, b))

    def pair(cond):
        """(byte offset in the blob of the lo code) of an x pair of a regular node whose half has a present slot."""
        for n in np.flatnonzero(regular):
            for hlf in range(2):
                lo_, hi_ = int(q[n, 2 * hlf]), int(q[n, 2 * hlf + 1])
                if (present[n, hlf] or present[n, 2 + hlf]) and cond(lo_, hi_):
                    return on + 32 * n + 16 + 2 * hlf
        raise ValueError("no pair to mutate")

    def bump(off, by):
        def edit(b):
            b[off] = np.uint8(int(b[off]) + by)
        return edit

    mutated("upper code one smaller", ("box",), bump(pair(lambda l, u: u > 0) + 1, -1))
    mutated("lower code one larger", ("box",), bump(pair(lambda l, u: l < 255), 1))
    mutated("upper code one larger", ("tight",), bump(pair(lambda l, u: u < 255) + 1, 1))
    rec = np.flatnonzero(prims.any(axis=1))
    s0, s1 = int(rec[0]), int(rec[-1])
    assert s0 // 4 != s1 // 4

    def swap(b):
        a = b[op + 48 * s0:op + 48 * s0 + 48].copy()
        b[op + 48 * s0:op + 48 * s0 + 48] = b[op + 48 * s1:op + 48 * s1 + 48]
        b[op + 48 * s1:op + 48 * s1 + 48] = a

    def copy(b):
        b[op + 48 * s0:op + 48 * s0 + 48] = b[op + 48 * s1:op + 48 * s1 + 48]

    mutated("two leaf records of different blocks swapped", ("box",), swap)
    mutated("one leaf record copied over another", ("prims",), copy)

    def word(off, fn):
        def edit(b):
            w = b[off:off + 4].view("<u4")
            w[0] = np.uint32(fn(int(w[0])) & 0xFFFFFFFF)
        return edit

    inner = np.flatnonzero(regular & (first >= 0))
    deep = int(inner[-1])                                    # a node with a node block, as far from the root as there is
    mutated("first moved by 2", ("topology",), word(on + 32 * deep + 12, lambda w: w + 2))
    mutated("first set to 0 (a cycle)", ("topology",), word(on + 32 * deep + 12, lambda w: 0))
    child = int(first[deep]) + int(np.flatnonzero(present[deep])[0])

    def kill(b):
        b[on + 32 * child:on + 32 * child + 32] = np.frombuffer(DEAD_BYTES, np.uint8)

    def zero_dead(b):
        b[on + 32:on + 64] = 0

    mutated("live child replaced by the dead pattern", ("topology",), kill)
    mutated("dead slot zeroed", ("topology",), zero_dead)
    mutated("x-step exponent bits of one origin incremented", ("box", "tight"), word(on + 32 * deep, lambda w: w + 1))
    mutated("one anc entry changed", ("anc",), word(oa + 4 * (S - 4), lambda w: w + 1))
    mutated("height decremented", ("topology",), word(32, lambda w: w - 1))
    mutated("one vertex word changed", ("header",), word(256 + 4 * 7, lambda w: w ^ 0x00010000))
    mutated("pad halved", ("header",), word(52, lambda w: _f32_bits(_bits_f32(w) * _F32(0.5))))
    return res


def plain_grid(n0, n1, relief=0.0, origin=(0.0, 0.0), dx=30.0, seed=3):
    """(vert_grid, n0, n1) of a regular grid with uniform random relief (none: a flat DEM)."""
    rng = np.random.default_rng(seed)
    x = (origin[0] + np.arange(n1) * dx).astype(np.float32)
    y = (origin[1] + (n0 - 1 - np.arange(n0)) * dx).astype(np.float32)
    xx, yy = np.meshgrid(x, y)
    z = (500.0 + relief * rng.random((n0, n1))).astype(np.float32)
    buf = np.zeros(3 * n0 * n1 + 16, np.float32)
    buf[0:3 * n0 * n1:3], buf[1:3 * n0 * n1:3], buf[2:3 * n0 * n1:3] = xx.ravel(), yy.ravel(), z.ravel()
    return buf, n0, n1


def badmap_mutations(blob):
    """The same for a valid blob that carries a bad-quad bitmap with set and unset cells: [(name, kinds, mutated copy)]."""
    src = _as_u8(blob).copy()
    h = decode(src)["hdr"]
    assert h["flags"] == HZ_BLOB_BAD_MAP
    ob, nbytes = h["off_bad"], h["bad_nb"] * h["bad_nb"] // 8
    bits = np.unpackbits(src[ob:ob + nbytes], bitorder="little")
    res = []

    def mutated(name, edit):
        b = src.copy()
        edit(b)
        res.append((name, ("badmap",), b))

    def flip(cell):
        def edit(b):
            b[ob + cell // 8] ^= np.uint8(1 << (cell % 8))
        return edit

    def word(off, fn):
        def edit(b):
            w = b[off:off + 4].view("<u4")
            w[0] = np.uint32(fn(int(w[0])) & 0xFFFFFFFF)
        return edit

    mutated("a set bitmap cell cleared", flip(int(np.flatnonzero(bits == 1)[0])))
    if (bits == 0).any():
        mutated("an unset bitmap cell set", flip(int(np.flatnonzero(bits == 0)[0])))
    mutated("n_flipped incremented", word(140, lambda w: w + 1))
    mutated("HEIGHT_FIELD set beside BAD_MAP", word(136, lambda w: w | HZ_BLOB_HEIGHT_FIELD))
    mutated("BAD_MAP cleared", word(136, lambda w: 0))
    mutated("bad_sx scaled", word(164, lambda w: _f32_bits(_bits_f32(w) * _F32(1.5))))
    return res
