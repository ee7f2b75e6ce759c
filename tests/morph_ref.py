"""numpy float32 restatement of include/urt.h urt_morph_vertices (csrc/morph.hip k_morph) and of the canonical morph plan
(csrc/morph_plan.cpp), operation for operation: one float32 rounding per operation, evaluated as written, no fma but the two of
urt_math.h's dot().  Test helper only (not a conftest): tests/test_morph_ref.py checks it against float64 morphing and on hand-made
cases, tests/test_gpu_morph.py checks the library against it bit for bit.

For served vertex i, p = rest position and n = rest normal; over its entries e sequentially in plan order (vertex, then target, then
input position), with w = weights[e.target]: the entry is LIVE when w != 0 (a NaN weight is live); a live entry does
    p.r = p.r + w * e.dp[r]        n.r = n.r + w * e.dn[r]
and an entry that is not live does nothing at all.  With normalize: L2 = fma(n.z, n.z, fma(n.y, n.y, n.x*n.x)); the normal is
n * (1 / sqrt(L2)) when L2 > 0 and finite, else n as it is."""
import numpy as np

from skin_ref import fma32

F = np.float32
DELTA_DT = np.dtype([("vertex", "<i4"), ("target", "<i4"), ("dp", "<f4", (3,)), ("dn", "<f4", (3,))])      # urt_MorphDelta, 32 bytes
BLOCK = 256              # csrc/morph.h kMorphBlock
MAX_TARGETS = 4096


def deltas_array(vertex, target, dp, dn=None):
    """Parallel arrays -> an array of urt_MorphDelta."""
    d = np.zeros(len(vertex), DELTA_DT)
    d["vertex"], d["target"], d["dp"] = vertex, target, np.asarray(dp, F).reshape(-1, 3)
    if dn is not None:
        d["dn"] = np.asarray(dn, F).reshape(-1, 3)
    return d


def plan(deltas, first, count):
    """The canonical plan: (ranges [count, 2] i32, order [n_deltas] i32, (n_entries, max_valence, n_touched)).  order sorts the input
    delta numbers by vertex, then target, then input position; ranges[v - first] = (start, length) into order."""
    d = np.asarray(deltas, DELTA_DT).reshape(-1)
    order = np.lexsort((np.arange(len(d)), d["target"], d["vertex"])).astype(np.int32)       # (the last key is the primary one)
    length = np.bincount(d["vertex"].astype(np.int64) - first, minlength=count).astype(np.int32)[:count] if len(d) else np.zeros(count, np.int32)
    start = (np.cumsum(length) - length).astype(np.int32)
    ranges = np.stack([start, length], axis=1).astype(np.int32).reshape(count, 2)
    return ranges, order, (len(d), int(length.max()) if count else 0, int((length > 0).sum()))


def morph(rest_vertices, rest_normals, deltas, first, count, weights, normalize=False):
    """(positions [count, 3] f32, normals [count, 3] f32 or None when rest_normals is None) of the served vertices."""
    d = np.asarray(deltas, DELTA_DT).reshape(-1)
    w_all = np.asarray(weights, F).reshape(-1)
    ranges, order, (_, max_valence, _) = plan(d, first, count)
    p = np.array(np.asarray(rest_vertices, F).reshape(-1, 3)[first: first + count])
    n = None if rest_normals is None else np.array(np.asarray(rest_normals, F).reshape(-1, 3)[first: first + count])
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(max_valence):                         # entry position k of every vertex at once
            has = ranges[:, 1] > k
            e = order[np.where(has, ranges[:, 0] + k, 0)]
            w = w_all[d["target"][e]]
            live = (has & (w != 0))[:, None]                 # (a NaN compares unequal: live)
            wk = w[:, None]
            p = np.where(live, (p + (wk * d["dp"][e]).astype(F)).astype(F), p)
            if n is not None:
                n = np.where(live, (n + (wk * d["dn"][e]).astype(F)).astype(F), n)
        if n is not None and normalize:
            l2 = fma32(n[:, 2], n[:, 2], fma32(n[:, 1], n[:, 1], n[:, 0] * n[:, 0]))
            ok = (l2 > 0) & np.isfinite(l2)
            inv = (F(1.0) / np.sqrt(np.where(ok, l2, F(1.0)).astype(F))).astype(F)
            n = np.where(ok[:, None], (n * inv[:, None]).astype(F), n)
    return p.astype(F), None if n is None else n.astype(F)


def morph64(rest_vertices, deltas, first, count, weights):
    """Positions of the served vertices in float64, and the bound of the float32 evaluation's error per component:
    (2V + 1) * 2^-24 * (|P_r| + sum_live |w| |dp_r|) for a vertex of V live entries — each live entry rounds twice (the product, the
    sum), every rounding is relative to a partial result no larger than that sum (to first order), and one more leaves room for the
    growth of the roundings themselves."""
    d = np.asarray(deltas, DELTA_DT).reshape(-1)
    w = np.asarray(weights, F).reshape(-1).astype(np.float64)[d["target"]]
    P = np.asarray(rest_vertices, F).reshape(-1, 3)[first: first + count].astype(np.float64)
    live = w != 0
    at = d["vertex"].astype(np.int64) - first
    pos, mag, V = P.copy(), np.abs(P), np.zeros(count)
    term = w[:, None] * d["dp"].astype(np.float64)
    np.add.at(pos, at[live], term[live])
    np.add.at(mag, at[live], np.abs(term[live]))
    np.add.at(V, at[live], 1.0)
    return pos, (2.0 * V[:, None] + 1.0) * 2.0 ** -24 * mag
