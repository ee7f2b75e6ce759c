"""numpy float32 restatement of the temporal reprojection of include/urt.h (urt_reproject, urt_blit_add_history), bit for bit.

Every operation is one float32 numpy ufunc, in the order the header writes it (one rounding per operation, no fma); the sums and matrix
rows are explicit elementwise chains (np.dot, @ and np.sum may reorder or fuse).  A test helper, not a conftest."""
import numpy as np

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _finite(a):
    return np.isfinite(a).all(axis=-1)


def reproject_ref(prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id, prev_world_to_clip, camera_to_world,
                  camera_inverse_projection, max_history=64.0, normal_threshold=0.9, plane_threshold=0.02):
    """The outputs of urt_reproject on (h, w, 4) float32 images (row 0 = bottom): {"color", "count", "motion"}, each (h, w, 4) float32."""
    prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id = (
        np.ascontiguousarray(a, dtype=F) for a in (prev_color, prev_count, prev_hit, prev_normal, prev_id, hit, normal, id))
    M = np.asarray(prev_world_to_clip, F).reshape(16)
    Cm = np.asarray(camera_to_world, F).reshape(16)
    Iv = np.asarray(camera_inverse_projection, F).reshape(16)
    mh, nt, pt = F(max_history), F(normal_threshold), F(plane_threshold)
    H, W = hit.shape[:2]
    with np.errstate(all="ignore"):
        k, z = normal[..., 3], hit[..., 3]
        Px, Py, Pz = hit[..., 0], hit[..., 1], hit[..., 2]
        nx, ny, nz = normal[..., 0], normal[..., 1], normal[..., 2]
        o = _bits(id[..., 0])
        # 1. class
        sky = k == F(0)
        surface = ~sky & np.isfinite(z) & (z > F(0)) & _finite(hit[..., :3]) & _finite(normal[..., :3])
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
        A = np.zeros((H, W, 4), F)
        for dx, dy, w in taps:
            tx, ty = x0 + dx, y0 + dy
            inside = window & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & (w > F(0))
            cxq, cyq = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            pc, col, m = prev_count[cyq, cxq, 0], prev_color[cyq, cxq], prev_normal[cyq, cxq]
            Q, oq = prev_hit[cyq, cxq], _bits(prev_id[cyq, cxq, 0])
            ok = inside & np.isfinite(pc) & (pc > F(0)) & _finite(col)
            nd = (nx * m[..., 0] + ny * m[..., 1]) + nz * m[..., 2]
            pd = np.abs((nx * (Q[..., 0] - Px) + ny * (Q[..., 1] - Py)) + nz * (Q[..., 2] - Pz))
            surf_ok = (m[..., 3] == k) & (oq == o) & np.isfinite(Q[..., 3]) & (Q[..., 3] > F(0)) & (nd >= nt) & (pd <= pt * z)
            ok &= np.where(sky, m[..., 3] == F(0), surf_ok)
            # 4. sums in tap order
            S = np.where(ok, S + w, S)
            for c in range(4):
                A[..., c] = np.where(ok, A[..., c] + w * col[..., c], A[..., c])
            N = np.where(ok, N + w * pc, N)
        hist = S >= F(0.01)
        color = np.zeros((H, W, 4), F)
        for c in range(4):
            color[..., c] = np.where(hist, A[..., c] / S, zero)
        cnt = np.where(hist, N / S, zero)
        if mh > F(0):
            cnt = np.where(hist, np.fmin(cnt, mh), zero)
        count = np.zeros((H, W, 4), F)
        count[..., 0] = cnt
        # 5. motion
        motion = np.zeros((H, W, 4), F)
        motion[..., 0] = np.where(window, qx - xs, zero)
        motion[..., 1] = np.where(window, qy - ys, zero)
        motion[..., 2] = np.where(window, S, zero)
    return {"color": color, "count": count, "motion": motion, "window": window, "surface": surface, "sky": sky}


def history_samples(n, max_history):
    """s of urt_blit_add_history for the count n."""
    n = np.asarray(n, F)
    mh = F(max_history)
    with np.errstate(all="ignore"):
        capped = np.fmin(n, mh - F(1.0)) if mh > F(0) else n
        return np.where(~np.isfinite(n) | (n < F(0)), F(0), capped).astype(F)


def blit_add_history_ref(src, dst, count, max_history=0.0):
    """(dst, count) after urt_blit_add_history(src, dst, count, max_history) on (h, w, 4) float32 images."""
    t, c = np.asarray(src, F), np.array(dst, F)
    s = history_samples(np.asarray(count, F)[..., 0], max_history)
    with np.errstate(all="ignore"):
        a = F(1.0) / (s + F(1.0))
        ia = F(1.0) - a
        out = np.empty_like(c)
        for ch in range(3):
            out[..., ch] = t[..., ch] * a + c[..., ch] * ia
        out[..., 3] = a * a + c[..., 3] * ia
        cnt = np.zeros_like(c)
        cnt[..., 0] = s + F(1.0)
    return out, cnt


def blit_add_ref(src, dst, sample):
    """dst after urt_blit_add(src, dst, sample) (the AdditionShader blend, csrc/kernels.hip k_blit_add)."""
    t, c = np.asarray(src, F), np.array(dst, F)
    with np.errstate(all="ignore"):
        a = F(1.0) / (F(sample) + F(1.0))
        ia = F(1.0) - a
        out = np.empty_like(c)
        for ch in range(3):
            out[..., ch] = t[..., ch] * a + c[..., ch] * ia
        out[..., 3] = a * a + c[..., 3] * ia
    return out


# ---- an analytic scene for the tests: the pixel-centre feature buffers of urt_render_aov, traced in float64 -------------------------
def default_objects():
    """A ground plane, three spheres and two walls (one of them partly covering another object), with sky above them."""
    return [("ground", 0), ("sphere", (-1.5, 1.0, 1.0), 1.0, 1), ("sphere", (1.8, 0.8, 3.0), 0.8, 2), ("sphere", (0.3, 2.6, 5.0), 0.7, 3),
            ("wall", 6.0, (-4.0, 4.0), (0.0, 3.0), 4), ("wall", 2.0, (2.5, 4.5), (0.0, 1.6), 5)]


def analytic_aovs(width, height, camera_to_world, camera_inverse_projection, objects=None):
    """(hit, normal, id) of the pixel-centre rays of a camera, as urt_render_aov lays them out: hit = (P, distance), normal = (n, kind),
    id = (object bits, primitive bits, 0, 0); a miss: (0, 0, 0, inf), (0, 0, 0, 0), (-1, -1, 0, 0) as int bits."""
    objects = default_objects() if objects is None else objects
    c2w = np.asarray(camera_to_world, np.float64).reshape(4, 4).T
    invp = np.asarray(camera_inverse_projection, np.float64).reshape(4, 4).T
    X, Y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    u = (X + 0.5) / width * 2 - 1
    v = (Y + 0.5) / height * 2 - 1
    e = np.stack([u, v, np.zeros_like(u), np.ones_like(u)], -1) @ invp.T
    d = e[..., :3] @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = c2w[:3, 3]
    best = np.full(u.shape, np.inf)
    nrm = np.zeros(u.shape + (3,))
    kind = np.zeros(u.shape)
    obj = np.full(u.shape, -1, np.int32)
    with np.errstate(all="ignore"):
        for ob in objects:
            if ob[0] == "ground":
                t = -o[1] / d[..., 1]
                n, k = np.broadcast_to([0.0, 1.0, 0.0], d.shape), 1
            elif ob[0] == "sphere":
                c, r = np.asarray(ob[1], np.float64), ob[2]
                oc = o - c
                b = d @ oc
                disc = b * b - (oc @ oc - r * r)
                t = -b - np.sqrt(disc)
                t = np.where(disc >= 0, t, np.inf)
                n = (o + t[..., None] * d - c) / r
                k = 2
            else:                                                        # wall: the plane z = zc, facing -z, inside an x / y window
                zc, (x0, x1), (y0, y1) = ob[1], ob[2], ob[3]
                t = (zc - o[2]) / d[..., 2]
                p = o + t[..., None] * d
                t = np.where((p[..., 0] >= x0) & (p[..., 0] <= x1) & (p[..., 1] >= y0) & (p[..., 1] <= y1), t, np.inf)
                n, k = np.broadcast_to([0.0, 0.0, -1.0], d.shape), 3
            t = np.where(t > 1e-4, t, np.inf)
            closer = t < best
            best = np.where(closer, t, best)
            nrm = np.where(closer[..., None], n, nrm)
            kind = np.where(closer, k, kind)
            obj = np.where(closer, ob[-1], obj)
    hitm = np.isfinite(best)
    P = np.where(hitm[..., None], o + np.where(hitm, best, 0)[..., None] * d, 0)
    hit = np.concatenate([P, best[..., None]], -1).astype(F)
    normal = np.concatenate([np.where(hitm[..., None], nrm, 0), kind[..., None]], -1).astype(F)
    ids = np.zeros(u.shape + (4,), np.int32)
    ids[..., 0] = obj
    ids[..., 1] = np.where(hitm, 0, -1)
    return hit, normal, ids.view(F)
