"""Inputs shared by the CPU and the GPU tests of urt_reproject_deformed: random images over the analytic scene of tests/reproject_ref.py
whose id texels carry random index slots and barycentrics, with random previous-position buffers that hit every dead case of the header
(slot -1, a slot past the end, an index outside the vertices, a NaN barycentric, a previous triangle without area, an object outside the
tables) next to triangles that lie on the scene's two walls, so that some deformed pixels do find their history.  Does not import the
library.  A test helper, not a conftest."""
import numpy as np

from reproject_motion_ref import IDENTITY
from reproject_ref import F, analytic_aovs

SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (96, 64)]                         # ragged against the 16 x 16 workgroup and the 8 x 8 wave tile
IDENTITY16 = np.eye(4, dtype=F).reshape(16)


def camera(w, h, position=(0.0, 1.0, -10.0), yaw_deg=0.0):
    """scenes.camera_matrices without the package: (_CameraToWorld, _CameraInverseProjection), 16 floats each, column-major."""
    f = 1.0 / np.tan(np.radians(81.0) * 0.5)
    cy, sy = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.diag([1.0, 1.0, -1.0])
    c2w[:3, 3] = position
    near, far = 0.3, 1000.0
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1] = f / (w / h), f
    proj[2, 2], proj[2, 3], proj[3, 2] = -(far + near) / (far - near), -2.0 * far * near / (far - near), -1.0
    return c2w.T.astype(F).reshape(16), np.linalg.inv(proj).T.astype(F).reshape(16)


def world_to_clip(c2w16, invp16):
    c2w = np.asarray(c2w16, np.float64).reshape(4, 4).T
    invp = np.asarray(invp16, np.float64).reshape(4, 4).T
    return (np.linalg.inv(invp) @ np.linalg.inv(c2w)).T.astype(F).reshape(16)


def random_matrix(rng, kind):
    if kind == "identity":
        return IDENTITY16.copy()
    m = np.eye(4)
    a = rng.normal() * (0.03 if kind == "small" else 1.0)
    m[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) * (1.0 if kind == "small" else rng.uniform(0.5, 2.0))
    m[:3, 3] = rng.normal(size=3) * (0.02 if kind == "small" else 0.5)
    out = m.T.astype(F).reshape(16)
    if kind == "nan":
        out[rng.integers(12)] = np.nan
    return out


def random_deform(rng, n_obj, nv=48, nt=24):
    """(prev_vertices, indices, matrices (n_obj, 16), deformed): vertices on the walls z = 6 and z = 2 of the analytic scene and anywhere,
    a few of them not finite; triangles with indices out of range and without area among them; objects 4 and 5 (the walls) mostly flagged."""
    pv = rng.normal(size=(nv, 3)).astype(F) * 2
    on6, on2 = np.arange(nv) % 4 < 2, np.arange(nv) % 4 == 2
    pv[on6] = np.stack([rng.uniform(-4, 4, on6.sum()), rng.uniform(0, 3, on6.sum()), np.full(on6.sum(), 6.0)], -1)
    pv[on2] = np.stack([rng.uniform(2.5, 4.5, on2.sum()), rng.uniform(0, 1.6, on2.sum()), np.full(on2.sum(), 2.0)], -1)
    pv[rng.integers(nv), rng.integers(3)] = np.nan
    pv[rng.integers(nv), rng.integers(3)] = np.inf
    ix = np.zeros((nt, 3), np.int32)
    for t in range(nt):
        pool = np.flatnonzero(on6) if t % 3 == 0 else np.flatnonzero(on2) if t % 3 == 1 else np.arange(nv)
        ix[t] = rng.choice(pool, 3, replace=False)
    ix[1, 1] = ix[1, 0]                                                        # no area
    ix[2] = ix[2, 0]
    ix[4, rng.integers(3)] = -1                                                # outside the vertices
    ix[5, rng.integers(3)] = nv
    ix[7, rng.integers(3)] = 2 ** 30
    ix[8, rng.integers(3)] = -2 ** 31
    kinds = ["identity", "small", "small", "wild", "nan"]
    mats = np.stack([random_matrix(rng, kinds[int(rng.integers(len(kinds)))]) for _ in range(n_obj)])
    flags = rng.choice(np.array([0, 1, 1, -5, 2 ** 31 - 1], np.int64), n_obj).astype(np.int32)
    for o in (4, 5):
        if o < n_obj and rng.random() < 0.8:
            flags[o], mats[o] = 1, random_matrix(rng, "identity" if rng.random() < 0.6 else "small")
    return pv, ix.reshape(-1), mats, flags


def random_table(rng, n):
    """A motion table: identity, small rigid, NaN and zero entries."""
    out = np.tile(IDENTITY, (n, 1))
    for e in out:
        r = rng.random()
        if r < 0.35:
            a = rng.normal() * 0.04
            e[:] = np.array([np.cos(a), 0, -np.sin(a), 0, 1, 0, np.sin(a), 0, np.cos(a), *(rng.normal(size=3) * 0.05)], F)
        elif r < 0.45:
            e[rng.integers(12)] = np.nan
        elif r < 0.5:
            e[:] = 0
    return out


def random_case(seed, w, h, move=True, n_slots=72):
    """Feature buffers of the analytic scene under two cameras with a random history; bad texels, kinds and object ids injected as
    tests/test_gpu_reproject_motion.py injects them; every id texel gets a random index slot (valid ones — any residue mod 3 —, -1, the
    last valid one, the first two past it, huge ones) and random barycentrics (a few NaN and inf)."""
    rng = np.random.default_rng(seed)
    cam_a = camera(w, h)
    cam_b = camera(w, h, position=(0.35, 1.2, -9.6), yaw_deg=4.0) if move else camera(w, h)
    prev = [a.copy() for a in analytic_aovs(w, h, *cam_a)]
    cur = [a.copy() for a in analytic_aovs(w, h, *cam_b)]
    color = (10.0 ** rng.uniform(-3, 2, (h, w, 4))).astype(F)
    count = np.zeros((h, w, 4), F)
    count[..., 0] = rng.choice([0.0, 1.0, 3.5, 17.0, 64.0, 200.0], (h, w))
    count[..., 1:] = rng.uniform(-1, 1, (h, w, 3))

    def inject(a, p, vals, comps):
        m = rng.random(a.shape[:2]) < p
        a[m, rng.choice(comps, m.sum())] = rng.choice(vals, m.sum())
    bad = [np.nan, np.inf, -np.inf]
    inject(color, 0.02, bad, [0, 1, 2, 3])
    inject(count, 0.02, bad + [-2.0], [0])
    for hit, normal, ids in (prev, cur):
        inject(hit, 0.02, bad + [-1.0, 0.0], [0, 1, 2, 3])
        inject(normal, 0.02, bad, [0, 1, 2])
        inject(normal, 0.03, [1.0, 2.0, 3.0, 0.0, 4.0, np.nan], [3])
        iv = ids.view(np.int32)
        m = rng.random(iv.shape[:2]) < 0.04
        iv[m, 0] += rng.choice([1, -1, 7, -9, 2 ** 30, -2 ** 31 + 5], m.sum()).astype(np.int32)
        slots = rng.integers(0, n_slots - 2, (h, w))
        special = rng.random((h, w))
        slots = np.where(special < 0.05, -1, np.where(special < 0.1, n_slots - 3, np.where(special < 0.14, n_slots - 2, np.where(
            special < 0.18, n_slots, np.where(special < 0.2, 2 ** 30, np.where(special < 0.22, -2 ** 31, np.where(special < 0.6, slots // 3 * 3, slots)))))))
        iv[..., 1] = slots.astype(np.int32)
        u = rng.uniform(0, 1, (h, w))
        v = rng.uniform(0, 1, (h, w)) * (1 - u)
        ids[..., 2], ids[..., 3] = u.astype(F), v.astype(F)
        inject(ids, 0.03, bad + [-0.5, 2.0], [2, 3])
    return rng, color, count, prev, cur, cam_a, cam_b


# (max_history, motion image wanted, normal_threshold, plane_threshold, moved_max_history, deform normal_threshold, (n_mesh, n_sphere), n_obj)
SETTINGS = [(0.0, True, 0.9, 0.02, 0.0, 0.5, (6, 4), 6),
            (64.0, False, 0.5, 0.2, 4.0, -1.0, (None, None), 6),
            (64.0, True, -1.0, 1e3, 8.0, -2.0, (6, None), 5),
            (32.0, True, 0.99, 0.05, 3.5, 0.0, (None, 4), 8),
            (16.0, False, 0.9, 0.02, 0.0, 0.99, (1, 1), 1)]


def settings_case(k, seed, w, h, move=True):
    """Everything one call needs for SETTINGS[k]: (images: color, count, prev x3, cur x3), (M, c2w, invp), params dict with the tables and
    deform, and whether the motion image is wanted."""
    mh, motion, nt, pt, mmh, dnt, (n_mesh, n_sphere), n_obj = SETTINGS[k]
    rng, color, count, prev, cur, cam_a, cam_b = random_case(seed, w, h, move)
    pv, ix, mats, flags = random_deform(rng, n_obj)
    params = dict(max_history=mh, normal_threshold=nt, plane_threshold=pt, moved_max_history=mmh,
                  mesh_motion=random_table(rng, n_mesh) if n_mesh else None, sphere_motion=random_table(rng, n_sphere) if n_sphere else None,
                  deform=(pv, ix, mats, flags, dnt))
    return (color, count, *prev, *cur), (world_to_clip(*cam_a), *cam_b), params, motion


def mesh_object_records(mats):
    """(n, 28) float32 rows of 112 bytes whose first 16 floats are the matrices: what prev_mesh_objects needs (the rest is not read)."""
    out = np.full((len(mats), 28), 123.0, F)
    out[:, :16] = mats
    return out
