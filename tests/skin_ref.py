"""numpy float32 restatement of include/urt.h urt_skin_vertices and urt_buffer_bounds (csrc/skin.hip k_skin / k_bounds), operation for
operation: one float32 rounding per operation, evaluated as written, no fma but the two of urt_math.h's dot().  Test helper only (not a
conftest): tests/test_skin_ref.py checks it against float64 skinning and on hand-made cases, tests/test_gpu_skin.py checks the library
against it bit for bit.

For vertex i with rest position P, rest normal N, bone indices j[0..3] and weights w[0..3]: term k is LIVE when w[k] != 0 (a NaN weight
is live) and 0 <= j[k] < n_bones; a term that is not live contributes +0.0 per component and its bone is not read.  Live term, with
a = bones[j[k]] (three columns of the linear part, then the translation) and r = 0, 1, 2:
    q.r = ((a[r]*P.x + a[3+r]*P.y) + a[6+r]*P.z) + a[9+r]      t_k.r = w[k]*q.r
    m.r = (a[r]*N.x + a[3+r]*N.y) + a[6+r]*N.z                  u_k.r = w[k]*m.r
position = ((t_0 + t_1) + t_2) + t_3; s = the same sum over u_k; L2 = fma(s.z, s.z, fma(s.y, s.y, s.x*s.x)); the normal is
s * (1 / sqrt(L2)) when L2 > 0 and finite, else s as it is."""
import numpy as np

F = np.float32
LDS_BONES = 256          # csrc/skin.h kSkinLdsBones: larger bone tables are gathered from global memory
BLOCK = 256              # csrc/skin.h kSkinBlock


def fma32(a, b, c):
    """float32 fma (urt_math.h f_fma): the float64 product is exact; the sum is rounded to odd in float64 (TwoSum error term) and then
    to float32, which rounds the exact a * b + c correctly.  A non-finite sum is what float64 makes of it."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s) & np.isfinite(err)
        odd = fin & (err != 0) & ((s.view(np.uint64) & 1) == 0)
        s = np.where(odd, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def live_terms(indices, weights, n_bones):
    j = np.asarray(indices, np.int32).reshape(-1, 4)
    w = np.asarray(weights, F).reshape(-1, 4)
    return (w != 0) & (j >= 0) & (j < n_bones)


def skin(rest_vertices, rest_normals, indices, weights, bones):
    """(positions [n, 3] f32, normals [n, 3] f32 or None when rest_normals is None)."""
    P = np.asarray(rest_vertices, F).reshape(-1, 3)
    N = None if rest_normals is None else np.asarray(rest_normals, F).reshape(-1, 3)
    j = np.asarray(indices, np.int32).reshape(-1, 4)
    w = np.asarray(weights, F).reshape(-1, 4)
    A = np.asarray(bones, F).reshape(-1, 12)
    live = live_terms(j, w, len(A))
    zero = np.zeros((len(P), 3), F)
    t, u = [], []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(4):
            a = A[np.where(live[:, k], j[:, k], 0)] if len(A) else np.zeros((len(P), 12), F)      # (a dead term's row is never used)
            wk = w[:, k: k + 1]
            q = ((a[:, 0:3] * P[:, 0:1] + a[:, 3:6] * P[:, 1:2]) + a[:, 6:9] * P[:, 2:3]) + a[:, 9:12]
            t.append(np.where(live[:, k: k + 1], wk * q, zero).astype(F))
            if N is not None:
                m = (a[:, 0:3] * N[:, 0:1] + a[:, 3:6] * N[:, 1:2]) + a[:, 6:9] * N[:, 2:3]
                u.append(np.where(live[:, k: k + 1], wk * m, zero).astype(F))
        pos = ((t[0] + t[1]) + t[2]) + t[3]
        if N is None:
            return pos.astype(F), None
        s = (((u[0] + u[1]) + u[2]) + u[3]).astype(F)
        l2 = fma32(s[:, 2], s[:, 2], fma32(s[:, 1], s[:, 1], s[:, 0] * s[:, 0]))
        ok = (l2 > 0) & np.isfinite(l2)
        inv = F(1.0) / np.sqrt(np.where(ok, l2, F(1.0)).astype(F))
        nrm = np.where(ok[:, None], s * inv[:, None].astype(F), s)
    return pos.astype(F), nrm.astype(F)


def skin64(rest_vertices, indices, weights, bones):
    """Positions in float64 (no rounding to speak of), and the bound of the float32 evaluation's error per component:
    13 * 2^-24 * sum_k |w_k| (sum_c |a_c| |P_c| + |a_9+r|) — each of the at most 13 roundings on the way to a component (5 for q, 1 for
    the weight, 3 for the sum, with room to spare for their growth) is relative to a partial result no larger than that sum."""
    P = np.asarray(rest_vertices, F).reshape(-1, 3).astype(np.float64)
    j = np.asarray(indices, np.int32).reshape(-1, 4)
    w = np.asarray(weights, F).reshape(-1, 4).astype(np.float64)
    A = np.asarray(bones, F).reshape(-1, 12).astype(np.float64)
    live = live_terms(indices, weights, len(A))
    pos = np.zeros((len(P), 3))
    mag = np.zeros((len(P), 3))
    for k in range(4):
        a = A[np.where(live[:, k], j[:, k], 0)]
        q = a[:, 0:3] * P[:, 0:1] + a[:, 3:6] * P[:, 1:2] + a[:, 6:9] * P[:, 2:3] + a[:, 9:12]
        qa = np.abs(a[:, 0:3]) * np.abs(P[:, 0:1]) + np.abs(a[:, 3:6]) * np.abs(P[:, 1:2]) + np.abs(a[:, 6:9]) * np.abs(P[:, 2:3]) + np.abs(a[:, 9:12])
        pos += np.where(live[:, k: k + 1], w[:, k: k + 1] * q, 0.0)
        mag += np.where(live[:, k: k + 1], np.abs(w[:, k: k + 1]) * qa, 0.0)
    return pos, 13.0 * 2.0 ** -24 * mag


def bounds(vertices, first=0, count=None):
    """(min [3] f32, max [3] f32, n) over the elements first .. first + count - 1 whose three components are finite; none: (+inf, -inf, 0)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    v = v[first: len(v) if count is None else first + count]
    v = v[np.isfinite(v).all(axis=1)]
    if not len(v):
        return np.full(3, np.inf, F), np.full(3, -np.inf, F), 0
    return v.min(axis=0), v.max(axis=0), len(v)


def two_bone_bend(vertices, angle_deg, axis=1):
    """A test pose: bone 0 the identity, bone 1 a rotation by angle_deg about the z axis through the centre of the vertices; weights blend
    from bone 0 at the bottom of `axis` to bone 1 at its top.  Returns (indices [n, 4] i32, weights [n, 4] f32, bones [2, 12] f32)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    lo, hi = v[:, axis].min(), v[:, axis].max()
    s = ((v[:, axis] - lo) / max(hi - lo, F(1e-6))).astype(F)
    idx = np.zeros((len(v), 4), np.int32)
    idx[:, 1] = 1
    wgt = np.zeros((len(v), 4), F)
    wgt[:, 0], wgt[:, 1] = F(1.0) - s, s
    c, sn = np.cos(np.radians(angle_deg)), np.sin(np.radians(angle_deg))
    centre = v.mean(axis=0).astype(np.float64)
    R = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
    b = centre - R @ centre
    bones = np.zeros((2, 12), F)
    bones[0] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    bones[1] = np.concatenate([R.T.reshape(-1), b]).astype(F)          # columns of R, then the translation
    return idx, wgt, bones
