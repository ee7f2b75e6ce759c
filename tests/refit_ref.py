"""numpy float32 restatement of the GPU refit of moved MeshObjects (csrc/refit.hip k_refit_tris / k_refit_level), operation for
operation, with fma emulated exactly, and the float64 checks of the property the traversal relies on: every child box contains the
triangles below it, with a margin.  Test helper only (not a conftest): tests/test_refit_ref.py checks the contract on the host builder's
trees, tests/test_gpu_refit_edges.py checks the library's refitted nodes against the restatement bit for bit.

The contract of a refit, given the topology read back before the move (nodes, leaf-order tri_index, mesh_root) and the new matrices:
- records: w_j = mul_m4(localToWorld, v_j, 1) (urt_math.h: the fma chain, lowest component first), r0 = w0, e1 = w1 - w0, e2 = w2 - w0;
- per moved MeshObject, ext = the largest FINITE |coordinate| of its w_j, and pad = ext * 2^-16 + 1e-30 (float32, in that order);
- bottom-up, a leaf child's box is the minNum / maxNum of its RECONSTRUCTED vertices r0, r0 + e1, r0 + e2 (float32 sums, as the
  traversal's triangle test sees them), an interior child's box the unpadded union of the two child boxes one level below; the pad is
  applied only where a box is written into a node;
- the nodes of MeshObjects that did not move, and every node's child codes and remaining words, are unchanged bit for bit."""
import numpy as np

from qnodes_ref import fma32, fmax, fmin

F = np.float32
INF = F(np.inf)
PAD_SCALE = F(1.52587890625e-5)         # 2^-16
PAD_FLOOR = F(1e-30)
# the variants of the restatement that tests/test_refit_ref.py runs as negative controls: each must fail the float64 checks
VARIANTS = ("no_pad", "other_pad", "scene_pad", "skip_deepest", "w_boxes_ulp")


def mul_m4(m, p):
    """urt_math.h mul_m4(m, x, y, z, 1): m [n, 16] or [16] (Unity memory order, column-major), p [n, 3] f32 -> [n, 3] f32."""
    m = np.asarray(m, F)
    if m.ndim == 1:
        m = np.broadcast_to(m, (len(p), 16))
    p = np.asarray(p, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([fma32(m[:, 12 + r], F(1), fma32(m[:, 8 + r], z, fma32(m[:, 4 + r], y, (m[:, r] * x).astype(F)))) for r in range(3)], axis=1)


def tri_mesh(mesh_objects, slots):
    """MeshObject of every index slot (the range [indices_offset, indices_offset + indices_count) that holds it), or -1."""
    off = np.asarray(mesh_objects["indices_offset"], np.int64)
    cnt = np.asarray(mesh_objects["indices_count"], np.int64)
    order = np.argsort(off, kind="stable")
    k = np.searchsorted(off[order], slots, side="right") - 1
    m = order[np.clip(k, 0, len(order) - 1)]
    ok = (k >= 0) & (slots >= off[m]) & (slots < off[m] + cnt[m])
    return np.where(ok, m, -1)


def records(sc, tri_index):
    """k_refit_tris for every leaf-order triangle: dict of w [n, 3, 3] (world vertices), r0, e1, e2 [n, 3] f32, mesh [n]."""
    slots = np.asarray(tri_index, np.int64)
    mesh = tri_mesh(sc.mesh_objects, slots)
    mats = np.asarray(sc.mesh_objects["localToWorldMatrix"], F).reshape(-1, 16)[np.maximum(mesh, 0)]
    idx = np.asarray(sc.indices, np.int64).reshape(-1)
    verts = np.asarray(sc.vertices, F).reshape(-1, 3)
    w = np.stack([mul_m4(mats, verts[idx[slots + j]]) for j in range(3)], axis=1)
    return {"w": w, "r0": w[:, 0], "e1": (w[:, 1] - w[:, 0]).astype(F), "e2": (w[:, 2] - w[:, 0]).astype(F), "mesh": mesh}


def reconstructed(rec):
    """The vertices as the triangle test and leaf_box see them: r0, r0 + e1, r0 + e2 (float32 sums) -> [n, 3, 3]."""
    r0 = rec["r0"]
    return np.stack([r0, (r0 + rec["e1"]).astype(F), (r0 + rec["e2"]).astype(F)], axis=1)


def exact_vertices(rec):
    """The same three vertices in float64 (sums of two float32: exact but for a 2^-53 relative rounding) -> [n, 3, 3]."""
    r0 = rec["r0"].astype(np.float64)
    return np.stack([r0, r0 + rec["e1"].astype(np.float64), r0 + rec["e2"].astype(np.float64)], axis=1)


def mesh_ext(rec, n_meshes):
    """Largest finite |coordinate| of the world vertices of each MeshObject (0 without one) -> [n_meshes] f32."""
    a = np.abs(rec["w"]).reshape(len(rec["w"]), 9)
    a = np.where(a < INF, a, F(0)).max(axis=1) if len(a) else np.zeros(0, F)     # (NaN < inf is false: skipped too)
    ext = np.zeros(n_meshes, F)
    keep = rec["mesh"] >= 0
    np.maximum.at(ext, rec["mesh"][keep], a[keep])
    return ext


def pad_of(ext):
    """blas_builder.cpp / refit.hip: ext * 2^-16 + 1e-30, rounded in float32 in that order."""
    return ((np.asarray(ext, F) * PAD_SCALE).astype(F) + PAD_FLOOR).astype(F)


def topology(nodes, mesh_root):
    """(children [n, 2] i32, MeshObject [n] (-1: unreachable), depth below its root [n] (-1)) of a forest of 64-byte nodes."""
    nodes = np.asarray(nodes, F).reshape(-1, 16)
    n = len(nodes)
    kids = nodes[:, 12:14].view(np.int32)
    node_mesh = np.full(n, -1, np.int64)
    depth = np.full(n, -1, np.int64)
    root = np.asarray(mesh_root, np.int64)
    cur = np.nonzero((root >= 0) & (root < n))[0]
    cur, cm = root[cur], cur
    d = 0
    while len(cur):
        assert (depth[cur] < 0).all(), "a node is reached twice"
        node_mesh[cur], depth[cur] = cm, d
        k = kids[cur].astype(np.int64)
        inner = k >= 0
        cur, cm = k[inner], np.repeat(cm[:, None], 2, axis=1)[inner]
        d += 1
    return kids, node_mesh, depth


def leaf_range(code):
    """leaf code -> (first leaf-order triangle, count)."""
    c = (~np.asarray(code, np.int64)) & 0xFFFFFFFF
    return c >> 3, (c & 7) + 1


def _leaf_boxes(pts, codes, lo_fn, hi_fn, init_lo, init_hi):
    """Per leaf code the min / max over the points pts[t] ([n, 3, 3]) of its triangles -> lo, hi [len(codes), 3]."""
    first, cnt = leaf_range(codes)
    lo = np.full((len(codes), 3), init_lo, pts.dtype)
    hi = np.full((len(codes), 3), init_hi, pts.dtype)
    for t in range(8):
        live = t < cnt
        if not live.any():
            break
        p = pts[np.where(live, first + t, 0)]                                  # [m, 3 vertices, 3 axes]
        for j in range(3):
            lo = np.where(live[:, None], lo_fn(lo, p[:, j]), lo)
            hi = np.where(live[:, None], hi_fn(hi, p[:, j]), hi)
    return lo, hi


def _bottom_up(kids, depth, select, leaf_box, union, levels=None, init=None):
    """Child boxes (unpadded) of the selected nodes, deepest level first: leaf children from leaf_box(codes), interior children from the
    union of the child's two boxes.  levels: the depths to process (default all); init: (lo, hi) to start from (default NaN).
    -> lo, hi [n, 2, 3] float64 (rows not processed keep init)."""
    n = len(kids)
    lo = np.full((n, 2, 3), np.nan) if init is None else init[0].copy()
    hi = np.full((n, 2, 3), np.nan) if init is None else init[1].copy()
    dmax = int(depth.max()) if n else -1
    for d in range(dmax, -1, -1):
        if levels is not None and d not in levels:
            continue
        sel = np.nonzero(select & (depth == d))[0]
        if not len(sel):
            continue
        for k in range(2):
            c = kids[sel, k].astype(np.int64)
            leaf = c < 0
            l, h = np.zeros((len(sel), 3)), np.zeros((len(sel), 3))
            if leaf.any():
                l[leaf], h[leaf] = leaf_box(c[leaf])
            if (~leaf).any():
                ci = c[~leaf]
                l[~leaf], h[~leaf] = union(lo[ci, 0], lo[ci, 1], hi[ci, 0], hi[ci, 1])
            lo[sel, k], hi[sel, k] = l, h
    return lo, hi


def moved_meshes(before, after):
    """refit's `moved`: the localToWorldMatrix changed (bit pattern) and the MeshObject has a triangle."""
    a = np.asarray(before.mesh_objects["localToWorldMatrix"], F).reshape(-1, 16).view(np.uint32)
    b = np.asarray(after.mesh_objects["localToWorldMatrix"], F).reshape(-1, 16).view(np.uint32)
    return (a != b).any(axis=1) & (np.asarray(after.mesh_objects["indices_count"]) >= 3)


def refit(sc, nodes, tri_index, mesh_root, moved, variant=None):
    """The nodes after the refit of the MeshObjects with moved[m] to the matrices of scene `sc` (the tree `nodes` read back before the move).
    variant: None (the contract) or one of VARIANTS, the negative controls:
      no_pad        boxes written without the pad;
      other_pad     each MeshObject padded with the pad of the next MeshObject (cyclic);
      scene_pad     every MeshObject padded with the largest pad of the scene;
      skip_deepest  the deepest interior level of the forest keeps its old boxes (its parents read those);
      w_boxes_ulp   leaf boxes from w0, w1, w2 instead of the reconstructed vertices, widened by one ulp instead of the pad.
    -> (nodes [n, 16] f32, pad [n_meshes] f32)."""
    nodes = np.asarray(nodes, F).reshape(-1, 16)
    out = nodes.copy()
    n_meshes = len(sc.mesh_objects)
    moved = np.asarray(moved, bool)
    rec = records(sc, tri_index)
    pad = pad_of(mesh_ext(rec, n_meshes))
    if variant == "no_pad":
        pad = np.zeros_like(pad)
    elif variant == "other_pad":
        pad = np.roll(pad, -1)
    elif variant == "scene_pad":
        pad = np.full_like(pad, pad.max() if len(pad) else 0)
    kids, node_mesh, depth = topology(nodes, mesh_root)
    select = (node_mesh >= 0) & moved[np.maximum(node_mesh, 0)]
    pts = rec["w"] if variant == "w_boxes_ulp" else reconstructed(rec)
    levels, init = None, None
    if variant == "skip_deepest":                    # (every node is interior: the deepest level of nodes is the deepest interior level)
        deepest = int(depth.max()) if len(depth) else -1
        levels = set(range(deepest))
        old = select & (depth == deepest)            # the skipped level's old boxes, as written (padded), stand in for what its parents read
        init = (np.stack([nodes[:, 0:3], nodes[:, 6:9]], axis=1).astype(np.float64), np.stack([nodes[:, 3:6], nodes[:, 9:12]], axis=1).astype(np.float64))
        init = (np.where(old[:, None, None], init[0], np.nan), np.where(old[:, None, None], init[1], np.nan))
    lo, hi = _bottom_up(kids, depth, select, lambda c: _leaf_boxes(pts, c, fmin, fmax, INF, -INF),
                        lambda l0, l1, h0, h1: (fmin(l0.astype(F), l1.astype(F)), fmax(h0.astype(F), h1.astype(F))), levels, init)
    w = np.nonzero(select)[0]
    if levels is not None:
        w = w[depth[w] < deepest]
    p = pad[node_mesh[w]][:, None]
    l, h = lo[w].astype(F), hi[w].astype(F)
    if variant == "w_boxes_ulp":
        out[w, 0:3], out[w, 3:6] = np.nextafter(l[:, 0], -INF), np.nextafter(h[:, 0], INF)
        out[w, 6:9], out[w, 9:12] = np.nextafter(l[:, 1], -INF), np.nextafter(h[:, 1], INF)
    else:
        out[w, 0:3], out[w, 3:6] = (l[:, 0] - p).astype(F), (h[:, 0] + p).astype(F)
        out[w, 6:9], out[w, 9:12] = (l[:, 1] - p).astype(F), (h[:, 1] + p).astype(F)
    return out, pad


def box_center_form(lo, hi):
    """urt_math.h box_center_form on [..., 3] f32 boxes -> (c, h); an inverted box gets h = -3e38."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    empty = ~(lo <= hi).all(axis=-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        m = ((F(0.5) * lo).astype(F) + (F(0.5) * hi).astype(F)).astype(F)
        r = ((fmax((m - lo).astype(F), (hi - m).astype(F)) * F(1.0000005)).astype(F) + F(1e-37)).astype(F)
    return np.where(empty, F(0), m).astype(F), np.where(empty, F(-3.0e38), r).astype(F)


def check_boxes(sc, nodes, tri_index, mesh_root, pad, tight=None):
    """The property the traversal relies on, in float64, on every child box of every MeshObject's tree:
      contain  every vertex r0, r0 + e1, r0 + e2 of every triangle below the box lies inside it;
      margin   ... at least half its MeshObject's pad inside, on every face;
      tight    (MeshObjects with tight[m] only) on every face the nearest such vertex lies at most pad (1 + 2^-6) inside: the box is the
               vertices' box padded with its own MeshObject's pad, not a looser one;
      centre   the centre / half-extent copy the trace kernels read (box_center_form) contains the box.
    -> dict of the number of failing faces per check, and the smallest margin in pads ("min_margin")."""
    nodes = np.asarray(nodes, F).reshape(-1, 16)
    rec = records(sc, tri_index)
    kids, node_mesh, depth = topology(nodes, mesh_root)
    pts = exact_vertices(rec)
    live = node_mesh >= 0
    vlo, vhi = _bottom_up(kids, depth, live, lambda c: _leaf_boxes(pts, c, np.minimum, np.maximum, np.inf, -np.inf),
                          lambda l0, l1, h0, h1: (np.minimum(l0, l1), np.maximum(h0, h1)))
    blo = np.stack([nodes[:, 0:3], nodes[:, 6:9]], axis=1)
    bhi = np.stack([nodes[:, 3:6], nodes[:, 9:12]], axis=1)
    n = np.nonzero(live)[0]
    vlo, vhi, blo, bhi = vlo[n], vhi[n], blo[n], bhi[n]
    p = np.asarray(pad, F)[node_mesh[n]].astype(np.float64)[:, None, None]
    ml = vlo - blo.astype(np.float64)                     # [m, 2, 3] how far inside the box the vertices lie
    mh = bhi.astype(np.float64) - vhi
    margins = np.concatenate([ml, mh], axis=2)
    res = {"contain": int((~(margins >= 0)).sum()), "margin": int((~(margins >= 0.5 * p)).sum())}
    res["min_margin"] = float(np.nanmin(margins / p)) if margins.size else np.inf
    if tight is not None:
        t = np.asarray(tight, bool)[node_mesh[n]]
        res["tight"] = int((~(margins[t] <= p[t] * (1 + 2.0 ** -6))).sum())
    c, h = box_center_form(blo, bhi)
    c, h = c.astype(np.float64), h.astype(np.float64)
    res["centre"] = int((~(c - h <= blo.astype(np.float64))).sum() + (~(c + h >= bhi.astype(np.float64))).sum())
    return res


def failures(res):
    """The number of failing faces over all checks of check_boxes."""
    return sum(v for k, v in res.items() if k != "min_margin")
