"""numpy float32 restatement of urt_reproject_objects (include/urt.h): urt_reproject with per-object motion tables, bit for bit.

As tests/reproject_ref.py: every operation is one float32 numpy ufunc in the order the header writes it; sums and matrix rows are explicit
elementwise chains.  A pixel that is not moved goes through exactly the operations of reproject_ref.  Does not import the library.
A test helper, not a conftest."""
import numpy as np

from reproject_ref import F, _bits, _finite

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)


def _table(t):
    if t is None:
        return None
    t = np.ascontiguousarray(t, dtype=F)
    assert t.ndim == 2 and t.shape[1] == 12 and t.shape[0] >= 1, t.shape
    return t


def apply_motion(entry, p):
    """P' of the header for one entry (12 floats) and points p (..., 3), in float32 with the header's operation order."""
    a = np.asarray(entry, F)
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        return np.stack([((a[r] * p[..., 0] + a[3 + r] * p[..., 1]) + a[6 + r] * p[..., 2]) + a[9 + r] for r in range(3)], -1)


def reproject_objects_ref(prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id, prev_world_to_clip, camera_to_world,
                          camera_inverse_projection, max_history=64.0, normal_threshold=0.9, plane_threshold=0.02, mesh_motion=None,
                          sphere_motion=None, moved_max_history=0.0):
    """The outputs of urt_reproject_objects on (h, w, 4) float32 images (row 0 = bottom); the tables are (n, 12) float32 arrays or None
    (handle 0).  {"color", "count", "motion"} plus the masks "window", "surface", "sky", "moved"."""
    prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id = (
        np.ascontiguousarray(a, dtype=F) for a in (prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id))
    M = np.asarray(prev_world_to_clip, F).reshape(16)
    Cm = np.asarray(camera_to_world, F).reshape(16)
    Iv = np.asarray(camera_inverse_projection, F).reshape(16)
    mh, nt, pt, mmh = F(max_history), F(normal_threshold), F(plane_threshold), F(moved_max_history)
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
        # the moved pixels: their table entry, P', n', L
        moved = np.zeros((H, W), bool)
        dead = np.zeros((H, W), bool)
        A = np.broadcast_to(IDENTITY, (H, W, 12)).copy()
        for kind, tab in tables.items():
            if tab is None:
                continue
            sel = surface & (k == kind)
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
        Px, Py, Pz = np.where(moved, Qx, Px), np.where(moved, Qy, Py), np.where(moved, Qz, Pz)
        nx, ny, nz = np.where(moved, mx, nx), np.where(moved, my, ny), np.where(moved, mz, nz)
        thr_n = np.where(moved, nt * L, nt)
        thr_p = np.where(moved, (pt * z) * L, pt * z)
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
    return {"color": color, "count": count, "motion": motion, "window": window, "surface": surface, "sky": sky, "moved": moved}


# ---- the move of the quality test (tests/test_gpu_reproject_motion.py), shared with its CPU coverage check ----------------------------
# Mixed test scene at 128 x 96 seen from a camera close enough that the two moved objects fill a fair share of the image: sphere 0 and
# MeshObject 1 (the icosphere) each take a step of about a tenth of a unit, the icosphere also turns by 4 degrees.
QUALITY_SIZE = (128, 96)
QUALITY_CAMERA = (3.0, 1.2, -7.5)
QUALITY_SPHERE, QUALITY_SPHERE_STEP = 0, (0.08, 0.0, 0.06)
QUALITY_MESH, QUALITY_MESH_POSE = 1, dict(translate=(2.58, 1.0, -0.94), scale=1.0, yaw_deg=-16.0)      # from (2.5, 1.0, -1.0), yaw -20
QUALITY_MIN_COVERAGE = 0.05
