"""numpy float32 restatement of the guide-driven upsampling of include/urt.h (urt_upsample), bit for bit.

Every operation is one float32 numpy ufunc, in the order the header writes it (one rounding per operation, no fma); the sums are explicit
elementwise chains, as in reproject_ref.py.  A test helper, not a conftest."""
import numpy as np

F = np.float32
WIDE_FALLBACK, SKY_FROM_ALBEDO = 1, 2


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _finite(a):
    return np.isfinite(a).all(axis=-1)


def low_grid_position(n_full, n_low):
    """Step 2 along one axis: q[X] = (((float)X + 0.5f) * (float)n_low) / (float)n_full - 0.5f."""
    X = np.arange(n_full, dtype=np.int64).astype(F)
    return ((X + F(0.5)) * F(n_low)) / F(n_full) - F(0.5)


def upsample_ref(low_color, low_hit, low_normal, low_id, hit, normal, id, low_count=None, albedo=None, normal_threshold=0.9,
                 plane_threshold=0.02, count_scale=1.0, flags=WIDE_FALLBACK):
    """The outputs of urt_upsample on float32 images (row 0 = bottom), the low_* ones (h, w, 4) and the others (H, W, 4):
    {"color", "count"} as (H, W, 4) float32, and as bool (H, W) maps "result", "stage2" (the result came from the 4 x 4 block), "surface",
    "sky" and "any_tap" (some texel of either stage, flag or not, passed the validity test: a pixel without it can have no result)."""
    low_color, low_hit, low_normal, low_id, hit, normal, id = (
        np.ascontiguousarray(a, dtype=F) for a in (low_color, low_hit, low_normal, low_id, hit, normal, id))
    h, w = low_color.shape[:2]
    H, W = hit.shape[:2]
    if low_count is None:
        low_n = np.ones((h, w), F)
    else:
        low_n = np.ascontiguousarray(low_count, dtype=F)[..., 0]
    nt, pt, cs = F(normal_threshold), F(plane_threshold), F(count_scale)
    with np.errstate(all="ignore"):
        k, z = normal[..., 3], hit[..., 3]
        Px, Py, Pz = hit[..., 0], hit[..., 1], hit[..., 2]
        nx, ny, nz = normal[..., 0], normal[..., 1], normal[..., 2]
        o = _bits(id[..., 0])
        # 1. class
        sky = k == F(0)
        surface = ~sky & np.isfinite(z) & (z > F(0)) & _finite(hit[..., :3]) & _finite(normal[..., :3])
        classed = surface | sky
        # 2. position on the low grid
        qx = np.broadcast_to(low_grid_position(W, w)[None, :], (H, W))
        qy = np.broadcast_to(low_grid_position(H, h)[:, None], (H, W))
        # 3. the bilinear footprint
        flx, fly = np.floor(qx), np.floor(qy)
        fx, fy = qx - flx, qy - fly
        gx, gy = F(1.0) - fx, F(1.0) - fy
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        ptz = pt * z
        zero = np.zeros((H, W), F)

        def valid(tx, ty):
            inside = classed & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
            col, m, nq = low_color[cy, cx], low_normal[cy, cx], low_n[cy, cx]
            Q, oq = low_hit[cy, cx], _bits(low_id[cy, cx, 0])
            ok = inside & np.isfinite(nq) & (nq > F(0)) & _finite(col)
            nd = (nx * m[..., 0] + ny * m[..., 1]) + nz * m[..., 2]
            pd = np.abs((nx * (Q[..., 0] - Px) + ny * (Q[..., 1] - Py)) + nz * (Q[..., 2] - Pz))
            surf_ok = (m[..., 3] == k) & (oq == o) & np.isfinite(Q[..., 3]) & (Q[..., 3] > F(0)) & (nd >= nt) & (pd <= ptz)
            return ok & np.where(sky, m[..., 3] == F(0), surf_ok), col, nq

        def gather(taps):
            S, N = zero.copy(), zero.copy()
            A = np.zeros((H, W, 4), F)
            any_ok = np.zeros((H, W), bool)
            for tx, ty, wgt, need_weight in taps:
                ok, col, nq = valid(tx, ty)
                any_ok |= ok
                if need_weight:
                    ok = ok & (wgt > F(0))
                S = np.where(ok, S + wgt, S)
                for c in range(4):
                    A[..., c] = np.where(ok, A[..., c] + wgt * col[..., c], A[..., c])
                N = np.where(ok, N + wgt * nq, N)
            return S, A, N, any_ok

        S1, A1, N1, any1 = gather([(x0, y0, gx * gy, True), (x0 + 1, y0, fx * gy, True), (x0, y0 + 1, gx * fy, True),
                                   (x0 + 1, y0 + 1, fx * fy, True)])
        res1 = classed & (S1 >= F(0.01))
        # 4. the 4 x 4 block, equal weights
        one = np.ones((H, W), F)
        S2, A2, N2, any2 = gather([(x0 - 1 + i, y0 - 1 + j, one, False) for j in range(4) for i in range(4)])
        stage2 = classed & ~res1 & (S2 >= F(1.0)) if flags & WIDE_FALLBACK else np.zeros((H, W), bool)
        result = res1 | stage2
        S = np.where(stage2, S2, S1)
        N = np.where(stage2, N2, N1)
        A = np.where(stage2[..., None], A2, A1)
        # 5. output
        color = np.zeros((H, W, 4), F)
        for c in range(4):
            color[..., c] = np.where(result, A[..., c] / S, zero)
        count = np.zeros((H, W, 4), F)
        count[..., 0] = np.where(result, (N / S) * cs, zero)
        if flags & SKY_FROM_ALBEDO and albedo is not None:
            alb = np.ascontiguousarray(albedo, dtype=F)
            take = result & sky
            color[..., :3] = np.where(take[..., None], alb[..., :3], color[..., :3])
    return {"color": color, "count": count, "result": result, "stage2": stage2, "surface": surface, "sky": sky, "any_tap": any1 | any2}


def bilinear_resize_ref(low, W, H):
    """The plain bilinear resize the quality test compares against: the q mapping and weights of steps 2 and 3, no validity tests; taps
    outside the image are left out and the weights renormalised.  float64; (h, w, 4) -> (H, W, 4)."""
    low = np.asarray(low, np.float64)
    h, w = low.shape[:2]
    qx = np.broadcast_to(low_grid_position(W, w).astype(np.float64)[None, :], (H, W))
    qy = np.broadcast_to(low_grid_position(H, h).astype(np.float64)[:, None], (H, W))
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    fx, fy = qx - x0, qy - y0
    S = np.zeros((H, W))
    A = np.zeros((H, W, low.shape[2]))
    for dx, dy, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        tx, ty = x0 + dx, y0 + dy
        inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        wgt = np.where(inside, wgt, 0.0)
        S += wgt
        A += wgt[..., None] * low[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
    return A / S[..., None]


# ---- seeded synthetic guide images: a few ids, kinds 0-3, planar and curved patches ---------------------------------------------------
def synthetic_guides(width, height, seed=0):
    """(hit, normal, id, albedo) of a made-up view that is the same function of the normalised pixel position on every grid, so that two
    grids of different sizes see the same surfaces: a sky band (kind 0), a ground plane (kind 1), a curved blob (kind 2) and two planar
    patches of kind 3 with different ids, one of them slanted.  Layouts as urt_render_aov's."""
    rng = np.random.default_rng(seed)
    cx, cy, r = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.6), rng.uniform(0.15, 0.3)
    split = rng.uniform(0.55, 0.8)
    u = ((np.arange(width, dtype=np.float64) + 0.5) / width)[None, :].repeat(height, 0)
    v = ((np.arange(height, dtype=np.float64) + 0.5) / height)[:, None].repeat(width, 1)
    kind = np.where(v > 0.8, 0, 1)
    obj = np.where(v > 0.8, -1, 0)
    P = np.stack([u * 4 - 2, np.zeros_like(u), v * 6], -1)
    n = np.broadcast_to([0.0, 1.0, 0.0], P.shape).copy()
    # two planar patches of kind 3 on the right
    patch = (u > split) & (v > 0.2) & (v <= 0.8)
    upper = patch & (v > 0.5)
    kind = np.where(patch, 3, kind)
    obj = np.where(patch, np.where(upper, 2, 1), obj)
    P = np.where(patch[..., None], np.stack([u * 4 - 2, v * 3, np.where(upper, 4.0 + (u - split) * 3.0, 5.0)], -1), P)
    slant = np.array([-3.0, 0.0, 4.0]) / 5.0
    n = np.where(patch[..., None], np.where(upper[..., None], slant, [0.0, 0.0, -1.0]), n)
    # a curved blob in front
    d2 = (u - cx) ** 2 + (v - cy) ** 2
    blob = d2 < r * r
    zz = np.sqrt(np.maximum(r * r - d2, 0.0))
    kind = np.where(blob, 2, kind)
    obj = np.where(blob, 3, obj)
    P = np.where(blob[..., None], np.stack([u * 4 - 2, v * 3, 3.0 - 4 * zz], -1), P)
    nb = np.stack([(u - cx), (v - cy), -zz], -1) / max(r, 1e-6)
    n = np.where(blob[..., None], nb, n)
    surf = kind != 0
    dist = np.where(surf, np.linalg.norm(P - [0.0, 1.0, -4.0], axis=-1), np.inf)
    hit = np.concatenate([np.where(surf[..., None], P, 0.0), dist[..., None]], -1).astype(F)
    normal = np.concatenate([np.where(surf[..., None], n, 0.0), kind[..., None].astype(np.float64)], -1).astype(F)
    ids = np.zeros((height, width, 4), np.int32)
    ids[..., 0] = obj
    ids[..., 1] = np.where(surf, 0, -1)
    albedo = np.concatenate([np.stack([u, v, 0.25 + 0.5 * u * v], -1), np.zeros_like(u)[..., None]], -1).astype(F)
    return hit, normal, ids.view(F), albedo


def synthetic_case(w, h, W, H, seed=0, sprinkle=True):
    """The inputs of one urt_upsample call on synthetic guides: a dict with low_color, low_count, low_hit, low_normal, low_id, hit, normal,
    id and albedo.  sprinkle: NaN / inf colours, zero, negative and NaN counts, and a few broken guide texels on either grid."""
    rng = np.random.default_rng(1000 + seed)
    low_hit, low_normal, low_id, _ = synthetic_guides(w, h, seed)
    hit, normal, ids, albedo = synthetic_guides(W, H, seed)
    low_color = rng.uniform(0.0, 2.0, (h, w, 4)).astype(F)
    low_count = np.zeros((h, w, 4), F)
    low_count[..., 0] = rng.integers(1, 9, (h, w)).astype(F)
    if sprinkle:
        def some(shape, p):
            return rng.uniform(0, 1, shape) < p
        low_color[some((h, w), 0.06), rng.integers(0, 4)] = np.nan
        low_color[some((h, w), 0.04), rng.integers(0, 4)] = np.inf
        low_count[some((h, w), 0.08), 0] = 0.0
        low_count[some((h, w), 0.03), 0] = -1.0
        low_count[some((h, w), 0.03), 0] = np.nan
        low_count[some((h, w), 0.02), 0] = np.inf
        if w >= 4 and h >= 4:
            low_count[1:3, 1:3, 0] = 0.0                            # a 2 x 2 hole: the pixels between its texels need stage 2
        low_hit[some((h, w), 0.04), 3] = np.nan
        hit[some((H, W), 0.03), rng.integers(0, 3)] = np.nan        # no class on the full grid
        normal[some((H, W), 0.02), 3] = 5.0                         # a kind the low grid does not have
        hit[some((H, W), 0.02), 3] = -1.0
    return {"low_color": low_color, "low_count": low_count, "low_hit": low_hit, "low_normal": low_normal, "low_id": low_id, "hit": hit,
            "normal": normal, "id": ids, "albedo": albedo}
