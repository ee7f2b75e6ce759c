"""numpy restatement of the normal cones of option "blas_cones" (csrc/cones.hip): the word layout, the ray word, the integer test of the
traversal loop (csrc/trace_device.h cone_ray_word / cone_skips) and a cone builder.  Test helper only (not a conftest):
tests/test_cones_ref.py checks the contract on this builder's words, tests/test_gpu_cones.py checks it on the words read back from the device
(the device builds in float32 and pads differently: its words need not equal these, they have to meet the same obligation).

The rule.  Child c of node n carries one dword of four signed bytes (ax, ay, az, T); a ray carries r = (round(127 d.x), round(127 d.y),
round(127 d.z), -127).  The child is skipped iff  ax rx + ay ry + az rz - 127 T > 0  (word 0 never skips).

The obligation.  If the test skips for a direction d with | |d| - 1 | <= 2^-10, then for every triangle (e1, e2) below the child, in real
arithmetic,  d . (e1 x e2) >= 2^-16 |e1| |e2|:  Moller-Trumbore's det = -d . (e1 x e2) (up to a few ulps of |e1| |e2| |d|, about 4e-7) is then
negative and the normative test rejects the triangle.

The margin.  Write A = (ax, ay, az) (integers), a~ = A / |A| (a unit vector: the cone is built around the QUANTIZED axis, so the axis costs
no error), u = d / |d|, n_i the unit normals, cos phi = min_i a~ . n_i, sin theta_i = |e1 x e2| / (|e1| |e2|), and
mu = max_i 2^-16 / (sin theta_i (1 - 2^-10)).  d . (e1 x e2) >= 2^-16 |e1| |e2| follows from u . n_i >= mu; with u . a~ = cos alpha, u . n_i >=
cos(alpha + phi), so it is enough that cos alpha >= sin(phi + kappa) with sin kappa = mu — valid only while phi + kappa < pi / 2, i.e.
cos phi > mu — and sin(phi + kappa) <= sin phi + mu =: s.  The ray bytes are R = 127 d + e with |e_k| <= 0.5001 (rounding to nearest plus
the float32 product), |e| <= 0.8663; A . R = 127 |A| |d| (a~ . u) + A . e, so a skip (A . R > 127 T) gives
a~ . u > (127 T - 0.8663 |A|) / (127 |A| (1 + 2^-10)), which is >= s as soon as
        T >= |A| (s (1 + 2^-10) + 0.8663 / 127).
T is that bound rounded up to an integer (one more step of at most 1 / 127 in cosine); a bound above 127 does not fit the byte: word 0.
With |A| about 127 the quantisation costs (0.87 + rounding up) / 127, about 0.014 in cosine."""
import numpy as np

DELTA = 2.0 ** -16            # d . G >= DELTA |e1| |e2|
LEN_TOL = 2.0 ** -10          # | |d| - 1 | <= LEN_TOL
RAY_ERR = 0.8663              # |R - 127 d| <= sqrt(3) * 0.5001


def decode_leaf(code):
    c = (~np.int64(code)) & 0xFFFFFFFF
    return int(c >> 3), int(c & 7) + 1


def child_ranges(nodes, mesh_root):
    """nodes[n, 16] f32, mesh_root[m] -> first[n, 2], count[n, 2]: the leaf-order triangle range below each child (contiguous: the builders
    emit the leaves of a subtree next to each other; asserted)."""
    code = np.ascontiguousarray(np.asarray(nodes, np.float32).reshape(-1, 16)[:, 12:14]).view(np.int32)
    n = len(code)
    first, count = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
    done = np.zeros(n, bool)
    for r in np.asarray(mesh_root, np.int64):
        if r < 0 or r >= n:
            continue
        stack = [int(r)]
        while stack:
            k = stack[-1]
            kids = [int(c) for c in code[k] if c >= 0 and not done[c]]
            if kids:
                stack.extend(kids)
                continue
            stack.pop()
            for j in range(2):
                c = int(code[k, j])
                if c < 0:
                    first[k, j], count[k, j] = decode_leaf(c)
                else:
                    lo = min(first[c, 0], first[c, 1])
                    hi = max(first[c, 0] + count[c, 0], first[c, 1] + count[c, 1])
                    assert hi - lo == count[c, 0] + count[c, 1], "a subtree's triangles are not contiguous in leaf order"
                    first[k, j], count[k, j] = lo, hi - lo
            done[k] = True
    return first, count


def pack(a, t):
    """(ax, ay, az, T) signed bytes -> uint32 words, ax in the lowest byte."""
    a, t = np.asarray(a, np.int64), np.asarray(t, np.int64)
    return ((a[..., 0] & 0xFF) | ((a[..., 1] & 0xFF) << 8) | ((a[..., 2] & 0xFF) << 16) | ((t & 0xFF) << 24)).astype(np.uint32)


def decode(words):
    """uint32 words -> (A[..., 3], T) as int64."""
    b = np.ascontiguousarray(np.asarray(words, np.uint32))[..., None].view(np.int8).astype(np.int64)
    return b[..., :3], b[..., 3]


def ray_bytes(d):
    """the ray word's first three bytes: round-to-nearest-even of the float32 product 127 d, clamped to [-127, 127] (minNum / maxNum: a NaN becomes a bound)."""
    with np.errstate(invalid="ignore"):
        v = np.float32(127.0) * np.asarray(d, np.float32)
    return np.rint(np.fmax(np.fmin(v, np.float32(127.0)), np.float32(-127.0))).astype(np.int64)


def skips(words, d):
    """the integer test: words[...] against directions d[..., 3] (broadcast) -> bool."""
    a, t = decode(words)
    r = ray_bytes(d)
    return (a * r).sum(axis=-1) - 127 * t > 0


def cone_word(e1, e2):
    """One child's word from the (e1, e2) [k, 3] of the triangles below it (float64 arithmetic; any float input)."""
    e1, e2 = np.asarray(e1, np.float64), np.asarray(e2, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = np.cross(e1, e2)
        gl = np.sqrt((g * g).sum(axis=1))
        l12 = np.sqrt((e1 * e1).sum(axis=1) * (e2 * e2).sum(axis=1))
        if not (np.all(gl > 0) and np.all(np.isfinite(gl)) and np.all(np.isfinite(l12))):
            return 0                                              # zero area, NaN, overflow
        nrm = g / gl[:, None]
        mu = (DELTA * l12 / gl).max() / (1.0 - LEN_TOL) * (1.0 + 1e-9)
        axis = nrm.sum(axis=0)
        al = np.sqrt((axis * axis).sum())
        if not al > 1e-6:
            return 0
        a = np.rint(127.0 * axis / al)
        an = np.sqrt((a * a).sum())
        c = (nrm @ (a / an)).min() - 1e-12                        # cos phi, padded down
        if not (c > mu and mu < 1.0):
            return 0                                              # phi + kappa >= pi / 2: mixed windings, wide spread, slivers
        s = np.sqrt(max(0.0, 1.0 - c * c)) + mu
        t = int(np.ceil(an * (s * (1.0 + LEN_TOL) + RAY_ERR / 127.0) * (1.0 + 1e-9)))
        if t > 127:
            return 0
    return int(pack(a.astype(np.int64), t))


def build_cones(nodes, mesh_root, e1, e2):
    """words[n, 2] uint32 for the tree `nodes` over the leaf-order triangle records (e1, e2) [n_tris, 3]."""
    first, count = child_ranges(nodes, mesh_root)
    w = np.zeros(first.shape, np.uint32)
    for k in range(len(first)):
        for j in range(2):
            if count[k, j] > 0:
                a, b = first[k, j], first[k, j] + count[k, j]
                w[k, j] = cone_word(e1[a:b], e2[a:b])
    return w


def world_edges(scene, tri_index):
    """(v0, e1, e2) [n_tris, 3] float32 of the leaf-order triangles: world-space v0, v1 - v0, v2 - v0 (float64 transform rounded to float32;
    the kernels' record differs from it by float32 rounding)."""
    v0 = np.zeros((len(tri_index), 3), np.float32)
    e1, e2 = np.zeros_like(v0), np.zeros_like(v0)
    slots = np.asarray(tri_index, np.int64)
    for mo in scene.mesh_objects:
        a, b = int(mo["indices_offset"]), int(mo["indices_offset"]) + int(mo["indices_count"])
        sel = np.nonzero((slots >= a) & (slots < b))[0]
        m = np.asarray(mo["localToWorldMatrix"], np.float64).reshape(4, 4).T
        p = [(scene.vertices[scene.indices[slots[sel] + i]].astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32) for i in range(3)]
        v0[sel], e1[sel], e2[sel] = p[0], p[1] - p[0], p[2] - p[0]
    return v0, e1, e2


def margin_ok(e1, e2, d):
    """float64: d . (e1 x e2) >= DELTA |e1| |e2| for triangles [k, 3] against directions d [m, 3] -> bool [m, k]."""
    e1, e2, d = np.asarray(e1, np.float64), np.asarray(e2, np.float64), np.asarray(d, np.float64)
    g = np.cross(e1, e2)
    l12 = np.sqrt((e1 * e1).sum(axis=1) * (e2 * e2).sum(axis=1))
    return d @ g.T >= DELTA * l12[None, :]


def boundary_directions(word, azimuths=8):
    """Unit directions stepped across one cone's boundary: a~ . u = t / |A| for t within +-4 steps of the word's T, at `azimuths` angles
    about the axis."""
    a, t = decode(np.uint32(word))
    a, t = a.astype(np.float64).reshape(3), int(np.asarray(t).reshape(-1)[0])
    an = np.sqrt((a * a).sum())
    u0 = a / an
    p = np.cross(u0, [1.0, 0.0, 0.0] if abs(u0[0]) < 0.9 else [0.0, 1.0, 0.0])
    p /= np.sqrt((p * p).sum())
    q = np.cross(u0, p)
    out = []
    for step in range(-4, 5):
        c = (t + step) / an
        if abs(c) > 1.0:
            continue
        s = np.sqrt(1.0 - c * c)
        for k in range(azimuths):
            ang = 2.0 * np.pi * (k + 0.37) / azimuths
            out.append(c * u0 + s * (np.cos(ang) * p + np.sin(ang) * q))
    return np.array(out).reshape(-1, 3)


def with_lengths(d):
    """d and d (1 +- 2^-10): the lengths the obligation covers."""
    d = np.asarray(d, np.float64)
    return np.concatenate([d, d * (1.0 + LEN_TOL), d * (1.0 - LEN_TOL)])


def check_obligation(words, first, count, e1, e2, common):
    """The obligation, for every child with a cone: wherever the integer test skips — over `common` [m, 3] and the child's own boundary
    directions, each at the three lengths — float64 d . G >= DELTA |e1| |e2| holds for every triangle of the child's range.
    -> (skips checked, children with a cone); raises AssertionError on the first violation."""
    common = with_lengths(common)
    n_skips = n_cones = 0
    for k in range(len(words)):
        for j in range(2):
            w = words[k, j]
            if w == 0:
                continue
            assert count[k, j] > 0 and first[k, j] >= 0, f"node {k} child {j}: a cone without a triangle range"
            n_cones += 1
            a, b = int(first[k, j]), int(first[k, j] + count[k, j])
            d = np.concatenate([common, with_lengths(boundary_directions(w))])
            sk = skips(w, d.astype(np.float32))
            if not sk.any():
                continue
            ds = d[sk].astype(np.float32).astype(np.float64)            # the float32 direction the kernel holds
            ok = margin_ok(e1[a:b], e2[a:b], ds)
            assert ok.all(), (f"node {k} child {j} word {int(w):#010x} (triangles {a}..{b - 1}): skipped {int((~ok).any(axis=1).sum())} of {len(ds)} "
                              f"directions although a triangle faces them (or by less than the margin)")
            n_skips += len(ds)
    return n_skips, n_cones


def own_axis_skips(words):
    """bool per child: the cone skips the direction along its own axis."""
    a, _ = decode(words)
    a = a.astype(np.float64)
    an = np.sqrt((a * a).sum(axis=-1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(an > 0, a / an, 0.0)
    return skips(words, d.astype(np.float32)) & (np.asarray(words) != 0)


CONE_MESHES = ("blob", "grid", "pair", "slivers", "zero")


def cone_mesh(kind):
    """(vertices, triangles) of the test meshes: a 24 x 20 uv_blob; an 8 x 8 flat grid; two layers of quads with opposite windings;
    needle slivers (some too thin for the margin) among ordinary triangles; a zero-area triangle among ordinary ones."""
    from unityraytracer_amd import scenes
    if kind == "blob":
        return scenes.uv_blob(24, 20)
    if kind == "grid":
        return scenes.grid_quad((-1.0, 0.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 8, (0.0, -1.0, 0.0))
    v, t = scenes.grid_quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), 3, (0.0, 0.0, 1.0))
    v, t = v.copy(), t.copy()
    if kind == "pair":
        back = v + np.array([0.0, 0.0, 0.5], np.float32)             # the same quads half a unit behind, wound the other way
        return np.concatenate([v, back]), np.concatenate([t, t[:, [0, 2, 1]] + len(v)])
    if kind == "slivers":
        extra_v, extra_t = [], []
        for i, width in enumerate((1e-2, 1e-4, 3e-5, 1e-5, 1e-6, 1e-8)):   # sin theta from 1e-2 down to far below 2^-16
            base = len(v) + len(extra_v)
            x = -0.9 + 0.3 * i
            extra_v += [(x, -0.5, 0.2), (x + 1.0, -0.5 + width, 0.2), (x + 2.0, -0.5, 0.2)]
            extra_t.append((base, base + 1, base + 2))
        return np.concatenate([v, np.array(extra_v, np.float32)]), np.concatenate([t, np.array(extra_t, np.int32)])
    if kind == "zero":
        base = len(v)
        extra_v = np.array([(0.1, 0.1, 0.3), (0.1, 0.1, 0.3), (0.4, 0.2, 0.3), (0.0, 0.0, 0.3), (0.5, 0.5, 0.3), (1.0, 1.0, 0.3)], np.float32)
        return np.concatenate([v, extra_v]), np.concatenate([t, np.array([(base, base + 1, base + 2), (base + 3, base + 4, base + 5)], np.int32)])
    raise ValueError(kind)


def cone_scene(kind, width=96, height=64, matrix=None):
    """One MeshObject of cone_mesh(kind), seen from Scene1's camera."""
    from unityraytracer_amd import scenes
    v, t = cone_mesh(kind)
    b = scenes.MeshSceneBuilder()
    m = matrix if matrix is not None else scenes.trs(translate=(0.0, 1.6, -5.0), scale=1.3, yaw_deg=20.0)
    b.add(v, t, m, scenes._params((0.7, 0.5, 0.3), (0.2, 0.2, 0.2), (0, 0, 0), 0.5))
    mo, vv, ii, nn, bvh = b.finish()
    return scenes.Scene(f"cones-{kind}", width, height, 4, 1, mesh_objects=mo, vertices=vv, indices=ii, normals=nn, mesh_bvh=bvh, sky=scenes.make_sky(64, 32))
