"""numpy restatement of what the in-place update of a DEFORMED MeshObject adds to the refit of a moved one (csrc/refit.hip,
csrc/scene_prep.cpp prepare_incremental).  Test helper only (not a conftest): tests/test_deform_ref.py checks it on hand-made trees,
tests/test_gpu_deform.py checks the library against it.  The box rule is tests/refit_ref.py's: the kernels do not distinguish a new
matrix from new vertices.

- span: the smallest and largest vertex the whole triangles of a MeshObject's index range refer to; a MeshObject is deformed (has its
  normals changed) when the dirty element range of _Vertices (_Normals) meets its span.  Conservative: a vertex inside the span that no
  index names counts.
- tri_norms: per leaf-order triangle the three object-space normals _Normals[_Indices[slot + j]] | 0, as a build writes them.
- tree cost, in float64, from the [lo, hi] nodes as stored (padded): per MeshObject the sum over its nodes and both children of
  area(child box) x (its triangle count for a leaf child, 1 for a node) / area(root box), the root box being the union of the root node's
  two child boxes.  Terms that are not finite add nothing; without nodes, or with a root box of zero or non-finite area, the cost is 0."""
import numpy as np

from refit_ref import leaf_range, refit, topology  # noqa: F401  (refit: the box rule, re-exported for the GPU test)

F = np.float32


def vertex_spans(mesh_objects, indices):
    """(lo, hi) [n_meshes] int64; lo > hi for a MeshObject without a triangle."""
    idx = np.asarray(indices, np.int64).reshape(-1)
    lo = np.zeros(len(mesh_objects), np.int64)
    hi = np.full(len(mesh_objects), -1, np.int64)
    for m, mo in enumerate(mesh_objects):
        off, cnt = int(mo["indices_offset"]), int(mo["indices_count"]) // 3 * 3
        if cnt > 0:
            lo[m], hi[m] = idx[off: off + cnt].min(), idx[off: off + cnt].max()
    return lo, hi


def dirty_range(old, new):
    """(first, last) element (row) at which two equally shaped arrays differ, bit for bit; None when they are equal."""
    a = np.ascontiguousarray(old).view(np.uint8).reshape(len(old), -1)
    b = np.ascontiguousarray(new).view(np.uint8).reshape(len(new), -1)
    rows = np.nonzero((a != b).any(axis=1))[0]
    return None if not len(rows) else (int(rows[0]), int(rows[-1]))


def meets(spans, rng):
    """The MeshObjects whose span meets the dirty range (None: none)."""
    lo, hi = spans
    if rng is None:
        return np.zeros(len(lo), bool)
    return (lo <= hi) & (lo <= rng[1]) & (hi >= rng[0])


def tri_norms(normals, indices, tri_index):
    """[n_tris, 3, 4] f32: n0 | 0, n1 | 0, n2 | 0 of every leaf-order triangle (tri_index: the slot of its first index)."""
    nrm = np.asarray(normals, F).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1)
    slots = np.asarray(tri_index, np.int64)
    out = np.zeros((len(slots), 3, 4), F)
    for j in range(3):
        out[:, j, :3] = nrm[idx[slots + j]]
    return out


def box_area(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])


def tree_cost(nodes, mesh_root, n_meshes=None):
    """(cost [n_meshes] float64, terms [n_meshes]: the number of summed terms, 2 per node)."""
    nodes = np.asarray(nodes, F).reshape(-1, 16)
    root = np.asarray(mesh_root, np.int64)
    n_meshes = len(root) if n_meshes is None else n_meshes
    kids, node_mesh, _ = topology(nodes, root)
    lo = np.stack([nodes[:, 0:3], nodes[:, 6:9]], axis=1)          # [n, child, 3]
    hi = np.stack([nodes[:, 3:6], nodes[:, 9:12]], axis=1)
    _, cnt = leaf_range(kids)
    weight = np.where(kids < 0, cnt, 1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        term = box_area(lo, hi) * weight                             # [n, 2]
    term = np.where(np.isfinite(term), term, 0.0)
    total = np.zeros(n_meshes)
    terms = np.zeros(n_meshes, np.int64)
    live = node_mesh >= 0
    np.add.at(total, node_mesh[live], term[live].sum(axis=1))
    np.add.at(terms, node_mesh[live], 2)
    cost = np.zeros(n_meshes)
    for m in range(n_meshes):
        r = root[m]
        if not (0 <= r < len(nodes)):
            continue
        with np.errstate(invalid="ignore"):
            area = box_area(np.fmin(lo[r, 0], lo[r, 1]), np.fmax(hi[r, 0], hi[r, 1]))
        if np.isfinite(area) and area > 0 and np.isfinite(total[m]):
            cost[m] = total[m] / area
    return cost, terms
