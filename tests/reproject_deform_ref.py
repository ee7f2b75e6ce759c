"""numpy float32 restatement of urt_reproject_deformed (include/urt.h): urt_reproject_objects with per-vertex motion for MeshObjects that
changed shape, bit for bit; and a small brute-force ray caster that makes the pixel-centre feature buffers (hit / normal / id with the
triangle's index slot and barycentrics) of a scene with meshes, so the CPU tests have real ones without a GPU.

As tests/reproject_motion_ref.py: every operation is one float32 numpy ufunc in the order the header writes it; sums and matrix rows are
explicit elementwise chains.  A pixel that is not deformed goes through exactly the operations of reproject_objects_ref.  Does not import
the library.  A test helper, not a conftest."""
import numpy as np

from reproject_motion_ref import IDENTITY, _table, reproject_objects_ref
from reproject_ref import F, _bits, _finite

DEFORM_NORMAL_THRESHOLD = 0.3                                                # include/urt.h URT_REPROJECT_DEFAULT_DEFORM_NORMAL_THRESHOLD


def matrices_of(mesh_objects):
    """The (n, 16) float32 localToWorldMatrix rows of a _MeshObjects list (records of 112 bytes whose first 16 floats are the matrix)."""
    a = np.ascontiguousarray(mesh_objects)
    assert a.nbytes % 112 == 0, a.nbytes
    return a.view(np.uint8).reshape(-1, 112)[:, :64].copy().view(F).reshape(-1, 16)


def previous_points(deform, o, i, u, v):
    """P', g, L of the header and the mask of pixels whose previous triangle is found and sound, for object ids o, index slots i and
    barycentrics u, v (arrays of one shape); deform = (prev_vertices, indices, matrices (n, 16), deformed, ...)."""
    pv = np.ascontiguousarray(deform[0], F).reshape(-1, 3)
    ix = np.ascontiguousarray(deform[1], np.int32).reshape(-1)
    mats = np.ascontiguousarray(deform[2], F).reshape(-1, 16)
    nv, ni, n = len(pv), len(ix), len(mats)
    with np.errstate(all="ignore"):
        ok = (i >= 0) & (i <= ni - 3)
        ic = np.where(ok, i, 0)
        ixp = np.concatenate([ix, np.zeros(3, np.int32)])                     # (fewer than three indices: nothing is ok, the pad is read)
        j = [ixp[ic + r] for r in range(3)]
        for r in range(3):
            ok = ok & (j[r] >= 0) & (j[r] < nv)
        A = [pv[np.clip(j[r], 0, nv - 1)] for r in range(3)]
        m = mats[np.clip(o, 0, n - 1)]
        V = [[((m[..., c] * A[r][..., 0] + m[..., 4 + c] * A[r][..., 1]) + m[..., 8 + c] * A[r][..., 2]) + m[..., 12 + c] for c in range(3)]
             for r in range(3)]
        w = (F(1.0) - u) - v
        P = [(V[0][c] * w + V[1][c] * u) + V[2][c] * v for c in range(3)]
        e1 = [V[1][c] - V[0][c] for c in range(3)]
        e2 = [V[2][c] - V[0][c] for c in range(3)]
        g = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        L = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        ok = ok & np.isfinite(P[0]) & np.isfinite(P[1]) & np.isfinite(P[2]) & (L > F(0)) & np.isfinite(L)
    return P, g, L, ok


def reproject_deformed_ref(prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id, prev_world_to_clip, camera_to_world,
                           camera_inverse_projection, max_history=64.0, normal_threshold=0.9, plane_threshold=0.02, mesh_motion=None,
                           sphere_motion=None, moved_max_history=0.0, deform=None):
    """The outputs of urt_reproject_deformed on (h, w, 4) float32 images (row 0 = bottom).  deform: None (NULL) or (prev_vertices (nv, 3),
    indices (ni,), matrices (n, 16) — matrices_of(prev_mesh_objects) —, deformed (n,) int32[, normal_threshold]).
    {"color", "count", "motion"} plus the masks "window", "surface", "sky", "moved", "deformed" (per-vertex path taken) and "kept" (a
    deformed pixel whose previous triangle was found and sound), "qx" / "qy" of step 2 and "P", the point each pixel projected."""
    if deform is None:
        out = reproject_objects_ref(prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id, prev_world_to_clip,
                                    camera_to_world, camera_inverse_projection, max_history, normal_threshold, plane_threshold, mesh_motion,
                                    sphere_motion, moved_max_history)
        out["deformed"] = out["kept"] = np.zeros(out["moved"].shape, bool)
        return out
    prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id = (
        np.ascontiguousarray(a, dtype=F) for a in (prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id))
    M = np.asarray(prev_world_to_clip, F).reshape(16)
    Cm = np.asarray(camera_to_world, F).reshape(16)
    Iv = np.asarray(camera_inverse_projection, F).reshape(16)
    mh, nt, pt, mmh = F(max_history), F(normal_threshold), F(plane_threshold), F(moved_max_history)
    dnt = F(deform[4] if len(deform) > 4 else DEFORM_NORMAL_THRESHOLD)
    flags = np.ascontiguousarray(deform[3], np.int32).reshape(-1)
    n_obj = len(flags)
    assert n_obj == len(np.ascontiguousarray(deform[2], F).reshape(-1, 16)) and n_obj >= 1
    tables = {F(3): _table(mesh_motion), F(2): _table(sphere_motion)}
    H, W = hit.shape[:2]
    with np.errstate(all="ignore"):
        k, z = normal[..., 3], hit[..., 3]
        Px, Py, Pz = hit[..., 0], hit[..., 1], hit[..., 2]
        nx, ny, nz = normal[..., 0], normal[..., 1], normal[..., 2]
        o = _bits(id[..., 0])
        # 1. class
        sky = k == F(0)
        surface = ~sky & np.isfinite(z) & (z > F(0)) & _finite(hit[..., :3]) & _finite(normal[..., :3])
        # the deformed pixels: the previous triangle, P', g, L
        tri = surface & (k == F(3))
        inside_o = (o >= 0) & (o < n_obj)
        dead = tri & ~inside_o
        deformed = tri & inside_o & (flags[np.clip(o, 0, n_obj - 1)] != 0)
        Dp, Dg, DL, sound = previous_points(deform, o, _bits(id[..., 1]), id[..., 2], id[..., 3])
        kept = deformed & sound
        dead |= deformed & ~sound
        # the moved pixels among the rest: their table entry, P', n', L
        moved = np.zeros((H, W), bool)
        A = np.broadcast_to(IDENTITY, (H, W, 12)).copy()
        for kind, tab in tables.items():
            if tab is None:
                continue
            sel = surface & (k == kind) & ~deformed & ~dead
            inside = (o >= 0) & (o < len(tab))
            dead |= sel & ~inside
            e = tab[np.clip(o, 0, len(tab) - 1)]
            ident = (e.view(np.int32) == IDENTITY.view(np.int32)).all(-1)
            mv = sel & inside & ~ident
            A[mv] = e[mv]
            moved |= mv
        a = [A[..., j] for j in range(12)]
        Qx = ((a[0] * Px + a[3] * Py) + a[6] * Pz) + a[9]
        Qy = ((a[1] * Px + a[4] * Py) + a[7] * Pz) + a[10]
        Qz = ((a[2] * Px + a[5] * Py) + a[8] * Pz) + a[11]
        mx = (a[0] * nx + a[3] * ny) + a[6] * nz
        my = (a[1] * nx + a[4] * ny) + a[7] * nz
        mz = (a[2] * nx + a[5] * ny) + a[8] * nz
        L = np.sqrt((mx * mx + my * my) + mz * mz)
        dead |= moved & ~(np.isfinite(Qx) & np.isfinite(Qy) & np.isfinite(Qz) & (L > F(0)) & np.isfinite(L))
        surface = surface & ~dead
        Px, Py, Pz = (np.where(kept, Dp[c], np.where(moved, q, p)) for c, q, p in ((0, Qx, Px), (1, Qy, Py), (2, Qz, Pz)))
        nx, ny, nz = (np.where(kept, Dg[c], np.where(moved, q, p)) for c, q, p in ((0, mx, nx), (1, my, ny), (2, mz, nz)))
        thr_n = np.where(kept, dnt * DL, np.where(moved, nt * L, nt))
        thr_p = np.where(kept, (pt * z) * DL, np.where(moved, (pt * z) * L, pt * z))
        moved = moved | kept
        # 2. projection: the surface point (w = 1) ...
        cx_s = ((M[0] * Px + M[4] * Py) + M[8] * Pz) + M[12]
        cy_s = ((M[1] * Px + M[5] * Py) + M[9] * Pz) + M[13]
        cw_s = ((M[3] * Px + M[7] * Py) + M[11] * Pz) + M[15]
        # ... or the pixel-centre direction (w = 0)
        xs = np.arange(W, dtype=np.int64).astype(F)[None, :].repeat(H, 0)
        ys = np.arange(H, dtype=np.int64).astype(F)[:, None].repeat(W, 1)
        u = ((xs + F(0.5)) / F(W)) * F(2.0) - F(1.0)
        v = ((ys + F(0.5)) / F(H)) * F(2.0) - F(1.0)
        e = [(Iv[r] * u + Iv[4 + r] * v) + Iv[12 + r] for r in range(3)]
        d = [(Cm[r] * e[0] + Cm[4 + r] * e[1]) + Cm[8 + r] * e[2] for r in range(3)]
        cx_k = (M[0] * d[0] + M[4] * d[1]) + M[8] * d[2]
        cy_k = (M[1] * d[0] + M[5] * d[1]) + M[9] * d[2]
        cw_k = (M[3] * d[0] + M[7] * d[1]) + M[11] * d[2]
        zero = np.zeros((H, W), F)
        cx = np.where(surface, cx_s, np.where(sky, cx_k, zero))
        cy = np.where(surface, cy_s, np.where(sky, cy_k, zero))
        cw = np.where(surface, cw_s, np.where(sky, cw_k, zero))
        qx = ((cx / cw + F(1.0)) * F(0.5)) * F(W) - F(0.5)
        qy = ((cy / cw + F(1.0)) * F(0.5)) * F(H) - F(0.5)
        window = (surface | sky) & (cw > F(0)) & (qx > F(-1.0)) & (qx < F(W)) & (qy > F(-1.0)) & (qy < F(H))
        # 3. bilinear taps
        flx = np.floor(np.where(window, qx, zero))
        fly = np.floor(np.where(window, qy, zero))
        fx = np.where(window, qx, zero) - flx
        fy = np.where(window, qy, zero) - fly
        gx, gy = F(1.0) - fx, F(1.0) - fy
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        taps = [(0, 0, gx * gy), (1, 0, fx * gy), (0, 1, gx * fy), (1, 1, fx * fy)]
        S, N = zero.copy(), zero.copy()
        Acc = np.zeros((H, W, 4), F)
        for dx, dy, w in taps:
            tx, ty = x0 + dx, y0 + dy
            inside = window & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & (w > F(0))
            cxq, cyq = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            pc, col, m = prev_count[cyq, cxq, 0], prev_color[cyq, cxq], prev_normal[cyq, cxq]
            Q, oq = prev_hit[cyq, cxq], _bits(prev_id[cyq, cxq, 0])
            ok = inside & np.isfinite(pc) & (pc > F(0)) & _finite(col)
            nd = (nx * m[..., 0] + ny * m[..., 1]) + nz * m[..., 2]
            pd = np.abs((nx * (Q[..., 0] - Px) + ny * (Q[..., 1] - Py)) + nz * (Q[..., 2] - Pz))
            surf_ok = (m[..., 3] == k) & (oq == o) & np.isfinite(Q[..., 3]) & (Q[..., 3] > F(0)) & (nd >= thr_n) & (pd <= thr_p)
            ok &= np.where(sky, m[..., 3] == F(0), surf_ok)
            # 4. sums in tap order
            S = np.where(ok, S + w, S)
            for c in range(4):
                Acc[..., c] = np.where(ok, Acc[..., c] + w * col[..., c], Acc[..., c])
            N = np.where(ok, N + w * pc, N)
        hist = S >= F(0.01)
        color = np.zeros((H, W, 4), F)
        for c in range(4):
            color[..., c] = np.where(hist, Acc[..., c] / S, zero)
        cnt = np.where(hist, N / S, zero)
        if mh > F(0):
            cnt = np.where(hist, np.fmin(cnt, mh), zero)
        if mmh > F(0):
            cnt = np.where(hist & moved, np.fmin(cnt, mmh), cnt)
        count = np.zeros((H, W, 4), F)
        count[..., 0] = cnt
        # 5. motion
        motion = np.zeros((H, W, 4), F)
        motion[..., 0] = np.where(window, qx - xs, zero)
        motion[..., 1] = np.where(window, qy - ys, zero)
        motion[..., 2] = np.where(window, S, zero)
    return {"color": color, "count": count, "motion": motion, "window": window, "surface": surface, "sky": sky, "moved": moved,
            "deformed": deformed, "kept": kept, "qx": qx, "qy": qy, "P": np.stack([Px, Py, Pz], -1)}


# ---- a brute-force ray caster: the pixel-centre feature buffers of urt_render_aov for meshes, spheres and the ground, in float64 --------
def cast_aovs(width, height, camera_to_world, camera_inverse_projection, mesh_objects=None, vertices=None, indices=None, normals=None,
              spheres=None, ground=True):
    """(hit, normal, id) as urt_render_aov lays them out: hit = (P, distance), normal = (n, kind: 1 ground, 2 sphere, 3 triangle), id =
    (object, index slot of the triangle's first index or -1 — int bits —, u, v); a miss: (0, 0, 0, inf), (0, 0, 0, 0), (-1, -1, 0, 0).
    Möller–Trumbore over every triangle of every MeshObject (records with localToWorldMatrix, indices_offset, indices_count; indices are
    positions in `vertices`); a triangle's normal is the interpolated vertex normal carried by the matrix's linear part.  spheres: records
    with position and radius, or an (n, 4) array."""
    c2w = np.asarray(camera_to_world, np.float64).reshape(4, 4).T
    invp = np.asarray(camera_inverse_projection, np.float64).reshape(4, 4).T
    X, Y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    e = np.stack([(X + 0.5) / width * 2 - 1, (Y + 0.5) / height * 2 - 1, np.zeros_like(X), np.ones_like(X)], -1) @ invp.T
    d = e[..., :3] @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    org = c2w[:3, 3]
    best = np.full(X.shape, np.inf)
    nrm = np.zeros(X.shape + (3,))
    kind = np.zeros(X.shape)
    obj = np.full(X.shape, -1, np.int32)
    slot = np.full(X.shape, -1, np.int32)
    bu, bv = np.zeros(X.shape), np.zeros(X.shape)

    def take(t, n, k, o, s=-1, u=0.0, v=0.0):
        nonlocal best, nrm, kind, obj, slot, bu, bv
        closer = (t > 1e-4) & (t < best)
        best = np.where(closer, t, best)
        nrm = np.where(closer[..., None], n, nrm)
        kind, obj, slot = np.where(closer, k, kind), np.where(closer, o, obj), np.where(closer, s, slot)
        bu, bv = np.where(closer, u, bu), np.where(closer, v, bv)

    with np.errstate(all="ignore"):
        if ground:
            take(-org[1] / d[..., 1], np.broadcast_to([0.0, 1.0, 0.0], d.shape), 1, -1)
        if spheres is not None and len(spheres):
            sp = np.asarray(spheres)
            pos = np.asarray(sp["position"], np.float64) if sp.dtype.names else np.asarray(sp[:, :3], np.float64)
            rad = np.asarray(sp["radius"], np.float64) if sp.dtype.names else np.asarray(sp[:, 3], np.float64)
            for s_i, (c, r) in enumerate(zip(pos, rad)):
                oc = org - c
                b = d @ oc
                disc = b * b - (oc @ oc - r * r)
                t = np.where(disc >= 0, -b - np.sqrt(disc), np.inf)
                take(t, (org + t[..., None] * d - c) / r, 2, s_i)
        if mesh_objects is not None:
            vv = np.asarray(vertices, np.float64).reshape(-1, 3)
            nn = np.asarray(normals, np.float64).reshape(-1, 3) if normals is not None else None
            ii = np.asarray(indices).reshape(-1)
            for m_i, mo in enumerate(mesh_objects):
                m = np.asarray(mo["localToWorldMatrix"], np.float64).reshape(4, 4).T
                first, cnt = int(mo["indices_offset"]), int(mo["indices_count"]) // 3 * 3
                for s_i in range(first, first + cnt, 3):
                    j = ii[s_i: s_i + 3]
                    v0, v1, v2 = (vv[j] @ m[:3, :3].T + m[:3, 3])
                    e1, e2 = v1 - v0, v2 - v0
                    p = np.cross(d, e2)
                    det = p @ e1
                    tv = org - v0
                    u = (p @ tv) / det
                    q = np.cross(tv, e1)
                    v = (d @ q) / det
                    t = (q @ e2) / det
                    t = np.where((det > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1), t, np.inf)      # front faces, as the reference culls
                    if not np.isfinite(t).any():
                        continue
                    if nn is not None:
                        n3 = (nn[j[0]] * (1 - u - v)[..., None] + nn[j[1]] * u[..., None] + nn[j[2]] * v[..., None]) @ m[:3, :3].T
                    else:
                        n3 = np.broadcast_to(np.cross(e1, e2), d.shape)
                    n3 = n3 / np.linalg.norm(n3, axis=-1, keepdims=True)
                    take(t, n3, 3, m_i, s_i, u, v)
    hitm = np.isfinite(best)
    P = np.where(hitm[..., None], org + np.where(hitm, best, 0)[..., None] * d, 0)
    hit = np.concatenate([P, best[..., None]], -1).astype(F)
    normal = np.concatenate([np.where(hitm[..., None], nrm, 0), kind[..., None]], -1).astype(F)
    ids = np.zeros(X.shape + (4,), np.int32)
    ids[..., 0], ids[..., 1] = obj, slot
    ids[..., 2], ids[..., 3] = bu.astype(F).view(np.int32), bv.astype(F).view(np.int32)
    return hit, normal, ids.view(F)


# ---- the move of the quality test (tests/test_gpu_reproject_deform.py), shared with its CPU coverage check -----------------------------
# Mixed test scene at 128 x 96 from a camera near the blob (MeshObject 0, uv_blob(12, 9)); the blob's bumps travel by a small phase step.
QUALITY_SIZE = (128, 96)
QUALITY_CAMERA = (-2.0, 1.5, -1.8)
QUALITY_MESH, QUALITY_BLOB = 0, (12, 9)
QUALITY_PHASE = (0.0, 0.6)                                                    # uv_blob's phase before and after the step
QUALITY_MIN_COVERAGE = 0.05
QUALITY_MIN_KEPT = 0.5
