"""numpy float32 restatement of the quantized triangle-BVH nodes of option "qnodes" (csrc/qnodes.hip k_qframe / k_quantize) and of the
traversal's slab test on them (csrc/trace_device.h make_qray / qnode_eval_ptr), operation for operation, with fma emulated exactly.
Test helper only (not a conftest): tests/test_qnodes_ref.py checks the contract on the host builder's trees, tests/test_gpu_qnodes.py
checks the library's read-back against it bit for bit."""
import numpy as np

F = np.float32
INF = F(np.inf)
# (cells across the union, cells below its lower corner, smallest cell relative to the largest |coordinate|) of csrc/qnodes.hip k_qframe
GRID = (65525.0, 3.0, 2.0 ** -20)
# the frame before it kept the margin: origin ON the lower corner, 65531 cells across.  The tests run their checks on it too, to show
# that they catch the faces it leaves without margin.
FORMER_GRID = (65531.0, 0.0, 0.0)


def fma32(a, b, c):
    """float32 fma (urt_math.h f_fma) in numpy: the float64 product is exact; the sum is rounded to odd in float64 (TwoSum error term)
    and then to float32, which rounds the exact a * b + c correctly."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    odd = (err != 0) & ((s.view(np.uint64) & 1) == 0)
    s = np.where(odd, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(F)


def fmin(a, b):
    """f_min on the device (__builtin_fminf): minNum, a NaN operand loses."""
    return np.fmin(np.asarray(a, F), np.asarray(b, F))


def fmax(a, b):
    return np.fmax(np.asarray(a, F), np.asarray(b, F))


def child_boxes(nodes):
    """nodes[n, 16] f32 ([lo0, hi0, lo1, hi1, child0, child1, ...]) -> lo[n, 2, 3], hi[n, 2, 3]."""
    n = np.asarray(nodes, F).reshape(-1, 16)
    return np.stack([n[:, 0:3], n[:, 6:9]], 1), np.stack([n[:, 3:6], n[:, 9:12]], 1)


def qframe(nodes, mesh_root, grid=GRID):
    """k_qframe: the ONE grid of the forest.  Contract: over the root nodes of the MeshObjects whose root is an interior node, the union
    [a, b] of their child boxes (only finite, non-inverted coordinates count; none at all -> [0, 0]); per axis
        cell = max(max((b - a) * (1 / 65525), max(|a|, |b|) * 2^-20), 1e-30) * 1.0000002     (float32, in this order)
        origin = a - 3 cell
    so that the union lies 3 cells above the origin and at least 4 cells below code 65535, and the rounding of a plane relative to the
    origin (2^-24 |origin|) stays below 1/16 cell.  quality = the smallest such MeshObject's extent along its longest axis, in cells.
    Returns (frame[2, 4] f32 = [origin.xyz, quality], [cell.xyz, 0])."""
    n = np.asarray(nodes, F).reshape(-1, 16)
    root = np.asarray(mesh_root, np.int64)
    r = root[(root >= 0) & (root < len(n))]
    lo, hi = child_boxes(n[r])                            # [m, 2, 3]
    ok = (lo <= hi) & (np.abs(lo) < INF) & (np.abs(hi) < INF)
    a = np.where(ok, lo, INF).reshape(-1, 3).min(axis=0) if len(r) else np.full(3, INF, F)
    b = np.where(ok, hi, -INF).reshape(-1, 3).max(axis=0) if len(r) else np.full(3, -INF, F)
    bad = ~(a <= b)
    a = np.where(bad, F(0), a).astype(F)
    b = np.where(bad, F(0), b).astype(F)
    ext = (b - a).astype(F)
    mag = np.maximum(np.abs(a), np.abs(b)).astype(F)
    cells_across, below, rel = grid
    cell = (np.maximum(np.maximum(ext * F(1.0 / cells_across), mag * F(rel)), F(1e-30)) * F(1.0000002)).astype(F)
    org = (a - F(below) * cell).astype(F)
    # quality
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = (fmax(hi[:, 0], hi[:, 1]) - fmin(lo[:, 0], lo[:, 1])).astype(F)       # [m, 3]
        cells = fmax(fmax(e[:, 0] / cell[0], e[:, 1] / cell[1]), e[:, 2] / cell[2]).astype(F)
    cells = cells[cells == cells]
    q = cells.min() if len(cells) else INF
    return np.array([[org[0], org[1], org[2], q], [cell[0], cell[1], cell[2], 0]], F)


MAX_CELL = 2.0 ** 43      # the traversal's 2^23 offset times S = cell / d (|1 / d| <= 1e18) must stay finite: 2^24 2^43 1e18 < 2^128


def in_use(frame, option):
    """Whether the traversal loop reads the quantized nodes (csrc/scene_prep.cpp requantize): option 1, or -1 with a quality of at least 1024
    cells, and in either case a grid whose cells are at most 2^43 on every axis."""
    return bool(frame[1, :3].max() <= MAX_CELL and (option == 1 or (option == -1 and frame[0, 3] >= 1024)))


def _q_lo(x, org, inv):
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.floor(((x - org).astype(F) * inv).astype(F)) - F(2)).astype(F)
    g = np.where(g >= 0, g, F(0))                          # (NaN -> 0: conservative)
    return np.minimum(g, F(65535)).astype(np.uint32)


def _q_hi(x, org, inv):
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.floor(((x - org).astype(F) * inv).astype(F)) + F(3)).astype(F)
    g = np.where(g <= 65535, g, F(65535))                  # (NaN -> 65535)
    return np.maximum(g, F(0)).astype(np.uint32)


def quantize(nodes, frame):
    """k_quantize: node n -> eight 32-bit words.  Contract: each child box [lo, hi] becomes grid codes
        lo' = clamp(floor((lo - origin) * (1 / cell)) - 2, 0, 65535),  hi' = clamp(floor((hi - origin) * (1 / cell)) + 3, 0, 65535)
    (outward, two cells of margin; NaN -> the whole grid), and an inverted box (lo > hi on some axis) becomes lo' = 65535, hi' = 0: never
    entered.  Words 0-2: child 0 lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16; words 3-5: child 1 the same; words 6-7: the two
    child codes, unchanged.  Returns uint32[n, 8]."""
    n = np.asarray(nodes, F).reshape(-1, 16)
    org = frame[0, :3].astype(F)
    inv = (F(1) / frame[1, :3].astype(F)).astype(F)
    lo, hi = child_boxes(n)
    a, b = _q_lo(lo, org, inv), _q_hi(hi, org, inv)       # [n, 2, 3]
    empty = (lo > hi).any(axis=2, keepdims=True)
    a = np.where(empty, np.uint32(65535), a)
    b = np.where(empty, np.uint32(0), b)
    w = np.zeros((len(n), 8), np.uint32)
    for c in range(2):
        w[:, 3 * c] = a[:, c, 0] | (a[:, c, 1] << 16)
        w[:, 3 * c + 1] = a[:, c, 2] | (b[:, c, 0] << 16)
        w[:, 3 * c + 2] = b[:, c, 1] | (b[:, c, 2] << 16)
    w[:, 6:8] = n[:, 12:14].view(np.uint32)
    return w


def quantized_nodes(nodes, mesh_root, grid=GRID):
    """(frame[2, 4], words[n, 8]): what urt_debug_read_scene_qnodes returns for this tree."""
    frame = qframe(nodes, mesh_root, grid)
    return frame, quantize(nodes, frame)


def decode(words):
    """uint32[n, 8] -> (lo[n, 2, 3], hi[n, 2, 3]) grid codes (int64)."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    lo, hi = np.zeros((len(w), 2, 3), np.int64), np.zeros((len(w), 2, 3), np.int64)
    for c in range(2):
        lo[:, c, 0], lo[:, c, 1] = w[:, 3 * c] & 0xFFFF, w[:, 3 * c] >> 16
        lo[:, c, 2], hi[:, c, 0] = w[:, 3 * c + 1] & 0xFFFF, w[:, 3 * c + 1] >> 16
        hi[:, c, 1], hi[:, c, 2] = w[:, 3 * c + 2] & 0xFFFF, w[:, 3 * c + 2] >> 16
    return lo, hi


def blas_rcp(d):
    """urt_math.h blas_rcp: 1 / d, with |d| < 1e-18 (+-0 included) taken as +-1e-18 by its sign bit."""
    d = np.asarray(d, F)
    with np.errstate(divide="ignore", over="ignore"):
        r = (F(1) / d).astype(F)
    neg = (d.view(np.uint32) >> 31) != 0
    return np.where(np.abs(d) < F(1e-18), np.where(neg, F(-1e18), F(1e18)), r).astype(F)


def ray_pad(o):
    """the per-ray pad of the triangle-BVH slab tests: 2^-16 max |o|."""
    return (np.abs(np.asarray(o, F)).max(axis=-1) * F(1.52587890625e-5)).astype(F)


def make_qray(o, d, frame):
    """make_qray: per ray and axis S = cell / d, and B+- = fma(-2^23, S, fma(origin, 1/d, -((o +- pad) / d))), so that the plane of grid
    code q lies at t = fma(2^23 + q, S, B).  Contract: t equals (origin + q cell - (o +- pad)) / d up to the rounding of B (at most one
    cell) and of the few float32 products (relative 2^-23): the quantizer's two cells cover both.  o, d: [m, 3] f32.  -> S, Bp, Bm [m, 3]."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    pad = ray_pad(o)[:, None]
    idir = blas_rcp(d)
    with np.errstate(over="ignore", invalid="ignore"):
        nop = (-((o + pad).astype(F) * idir)).astype(F)
        nom = (-((o - pad).astype(F) * idir)).astype(F)
        S = (frame[1, :3].astype(F) * idir).astype(F)
    org = np.broadcast_to(frame[0, :3].astype(F), o.shape)
    Bp = fma32(F(-8388608.0), S, fma32(org, idir, nop))
    Bm = fma32(F(-8388608.0), S, fma32(org, idir, nom))
    return S, Bp, Bm


def qnode_slabs(lo_codes, hi_codes, S, Bp, Bm, tbest):
    """qnode_eval_ptr for one child per ray: lo_codes / hi_codes [m, 3] grid codes; -> (tn, tf), entered iff tn <= tf.  Contract: tn =
    max over axes of the nearer plane and 0, tf = min over axes of the farther plane and tbest (minNum / maxNum: NaN loses), the planes
    at fma(2^23 + q, S, B+) for lo and fma(2^23 + q, S, B-) for hi."""
    ql = (F(8388608.0) + np.asarray(lo_codes, np.int64).astype(F)).astype(F)
    qh = (F(8388608.0) + np.asarray(hi_codes, np.int64).astype(F)).astype(F)
    a1, a2 = fma32(ql, S, Bp), fma32(qh, S, Bm)
    mn, mx = fmin(a1, a2), fmax(a1, a2)
    tn = fmax(fmax(mn[:, 0], mn[:, 1]), fmax(mn[:, 2], F(0)))
    tf = fmin(fmin(mx[:, 0], mx[:, 1]), fmin(mx[:, 2], np.asarray(tbest, F)))
    return tn, tf
