"""The quantized triangle-BVH nodes of option "qnodes" (csrc/qnodes.hip), checked on the host builder's trees through their numpy
restatement (tests/qnodes_ref.py; tests/test_gpu_qnodes.py checks the library's nodes against it bit for bit):
- every quantized child box holds its float box with two cells of margin on every face, the faces on the grid's corners included;
- the traversal's slab test on them (make_qray / qnode_eval_ptr, float32 with exact fma) enters every box that the exact ray enters,
  over millions of rays aimed at box faces, edges and corners: grazing, axis-parallel (components 0, -0 and below the 1e-18 clamp),
  from the world origin (no ray pad) and from 1e4 away, on forests near and far from the origin.
The frame the quantizer used before (origin on the union's lower corner) fails both on the lower-face scenes: the negative controls
below keep the checks honest."""
import numpy as np
import pytest

import qnodes_ref as Q
from unityraytracer_amd import debug_build_blas, scenes

F = np.float32

SCENES = {
    "mixed": lambda: scenes.mixed_test_scene(64, 40, blob=(40, 31)),
    "many_meshes": lambda: scenes.many_meshes_scene(64, 40),
    "config3": lambda: scenes.config3(64, 36),
    "deep_chain": lambda: scenes.deep_chain_scene(64, 40),
    **{k: (lambda k=k: scenes.qnode_edge_scene(k)) for k in scenes.QNODE_EDGE_KINDS if k != "axis"},
}
LOWER_FACE = ("floor", "wall_x", "wall_z")
MARGIN_TOL = 1.0 / 64      # the quantizer's own float32 rounding of (x - origin) / cell: < 65536 * 2^-23 cells


_trees = {}


def tree(name):
    if name not in _trees:
        sc = SCENES[name]()
        nodes, _, root, _, _ = debug_build_blas(sc.mesh_objects, sc.vertices, sc.indices)
        _trees[name] = (nodes, root)
    return _trees[name]


def margins(nodes, frame, words):
    """Per child box and face, how far (in cells, float64) the quantized plane lies OUTSIDE the float plane; inverted boxes are skipped.
    -> (lower faces [m, 3], upper faces [m, 3])."""
    lo, hi = Q.child_boxes(nodes)
    qlo, qhi = Q.decode(words)
    org, cell = frame[0, :3].astype(np.float64), frame[1, :3].astype(np.float64)
    keep = (lo <= hi).all(axis=2)
    lo, hi, qlo, qhi = lo[keep].astype(np.float64), hi[keep].astype(np.float64), qlo[keep], qhi[keep]
    return (lo - (org + qlo * cell)) / cell, ((org + qhi * cell) - hi) / cell


@pytest.mark.parametrize("name", list(SCENES))
def test_quantized_boxes_hold_the_float_boxes_with_two_cells(name):
    nodes, root = tree(name)
    frame, words = Q.quantized_nodes(nodes, root)
    ml, mh = margins(nodes, frame, words)
    assert ml.min() >= 2 - MARGIN_TOL and mh.min() >= 2 - MARGIN_TOL, (name, ml.min(), mh.min())
    # the grid's corners: some box face lies on the union's lower / upper corner on every axis, and keeps its margin there
    qlo, qhi = Q.decode(words)
    lo, hi = Q.child_boxes(nodes)
    live = (lo <= hi).all(axis=2)
    assert (qlo[live].min(axis=0) <= 1).all() and (qlo[live].min(axis=0) >= 0).all(), qlo[live].min(axis=0)
    assert (qhi[live].max(axis=0) <= 65533).all(), qhi[live].max(axis=0)       # the upper corner stays clear of the clamp too
    # child codes unchanged; inverted boxes never entered
    assert np.array_equal(words[:, 6:8], np.asarray(nodes, F)[:, 12:14].view(np.uint32))
    assert (qlo[~live] == 65535).all() and (qhi[~live] == 0).all()
    # the frame: origin 3 cells below the union, quality in cells
    assert np.isfinite(frame).all() and (frame[1, :3] > 0).all() and frame[0, 3] > 0


def test_inverted_and_degenerate_boxes():
    """A tree by hand: an inverted child box stays (65535, 0) whatever its coordinates; a root of a single point gets the 1e-30 cell."""
    node = np.zeros((1, 16), F)
    node[0, 0:6] = (0, 0, 0, 0, 0, 0)                              # child 0: a point at the origin
    node[0, 6:12] = (1, 1, 1, -1, -1, -1)                          # child 1: inverted
    node[0, 12:14] = np.array([-5, -6], np.int32).view(F)
    frame, words = Q.quantized_nodes(node, np.array([0], np.int32))
    assert np.array_equal(frame[1, :3], np.full(3, F(1e-30) * F(1.0000002), F))
    qlo, qhi = Q.decode(words)
    assert (qlo[0, 1] == 65535).all() and (qhi[0, 1] == 0).all()
    assert (qlo[0, 0] == 1).all() and (qhi[0, 0] == 6).all()       # 3 cells above the origin, widened by 2 below and 3 (ceil + 2) above
    ml, mh = margins(node, frame, words)
    assert ml.min() >= 2 - MARGIN_TOL and mh.min() >= 2 - MARGIN_TOL


@pytest.mark.parametrize("name", LOWER_FACE)
def test_the_former_frame_leaves_the_lower_faces_without_margin(name):
    """Negative control: with the origin ON the union's lower corner (the frame before), a face on that corner quantizes to
    floor(0) - 2 -> clamped to 0, i.e. onto the float plane itself."""
    nodes, root = tree(name)
    frame, words = Q.quantized_nodes(nodes, root, Q.FORMER_GRID)
    ml, _ = margins(nodes, frame, words)
    assert ml.min() < 0.5, ml.min()


# ---- the slab test ----------------------------------------------------------------------------------------------------------

def exact_enter(o, d, lo, hi, widen, tbest=np.inf):
    """float64: does the ray o + t d' (t in [0, tbest]) meet [lo - widen, hi + widen]?  d' = d with |d| < 1e-18 taken as +-1e-18 by its
    sign bit, as blas_rcp does for every slab test of the library (float nodes and quantized alike).  -> (enter, tn, tf)."""
    d = np.asarray(d, F)
    neg = (d.view(np.uint32) >> 31) != 0
    dd = np.where(np.abs(d) < F(1e-18), np.where(neg, -1e-18, 1e-18), d.astype(np.float64))
    o64 = o.astype(np.float64)
    w = np.asarray(widen, np.float64)[:, None]
    t1, t2 = (lo.astype(np.float64) - w - o64) / dd, (hi.astype(np.float64) + w - o64) / dd
    tn = np.maximum(np.minimum(t1, t2).max(axis=1), 0.0)
    tf = np.minimum(np.maximum(t1, t2).min(axis=1), tbest)
    return tn <= tf, tn, tf


def make_rays(rng, lo, hi, n):
    """n rays aimed at points on the faces, edges and corners of the boxes [lo, hi] ([n, 3] each, f32), in several families."""
    u = rng.random((n, 3))
    where = rng.integers(0, 3, (n, 3))                            # per axis: on lo, on hi, or inside
    p = np.where(where == 0, lo, np.where(where == 1, hi, lo + u * (hi - lo))).astype(np.float64)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fam = rng.integers(0, 6, n)
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    # grazing: one component tiny against the others
    g = fam == 1
    d[rows[g], ax[g]] *= 10.0 ** rng.uniform(-9, -2, g.sum())
    # axis-parallel: one or two components exactly 0 / -0 / below the 1e-18 clamp
    a = fam == 2
    tiny = rng.choice(np.array([0.0, -0.0, 1e-19, -1e-19, 1e-30, -3e-25]), size=(n, 3))
    d[rows[a], ax[a]] = tiny[rows[a], 0]
    two = a & (rng.random(n) < 0.5)
    d[rows[two], (ax[two] + 1) % 3] = tiny[rows[two], 1]
    d = d.astype(F)
    # origins: near (1e-3 .. 1e2 back along the ray), the world origin (pad 0), 1e4 away
    t = 10.0 ** rng.uniform(-3, 2, n)
    o = p - t[:, None] * d.astype(np.float64)
    wo = fam == 3
    o[wo] = 0.0
    dir0 = p[wo] / np.maximum(np.linalg.norm(p[wo], axis=1, keepdims=True), 1e-30)
    d[wo] = np.where(np.linalg.norm(p[wo], axis=1, keepdims=True) > 0, dir0, d[wo].astype(np.float64)).astype(F)
    far = fam == 4
    o[far] = p[far] - 1e4 * d[far].astype(np.float64)
    return o.astype(F), d


def slab_failures(nodes, root, grid=Q.GRID, n_rays=300_000, seed=0):
    """Rays (aimed at child boxes, those on the grid's corners first) that the exact ray enters but the quantized slab test rejects, with
    tbest = +inf and with tbest inside the exact segment.  -> (failures, rays checked)."""
    rng = np.random.default_rng(seed)
    frame, words = Q.quantized_nodes(nodes, root, grid)
    lo, hi = Q.child_boxes(nodes)
    qlo, qhi = Q.decode(words)
    lo, hi, qlo, qhi = lo.reshape(-1, 3), hi.reshape(-1, 3), qlo.reshape(-1, 3), qhi.reshape(-1, 3)
    live = np.nonzero((lo <= hi).all(axis=1) & np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1))[0]
    corner = live[((lo[live] == lo[live].min(axis=0)) | (hi[live] == hi[live].max(axis=0))).any(axis=1)]
    pick = np.where(rng.random(n_rays) < 0.5, rng.choice(corner, n_rays), rng.choice(live, n_rays))
    o, d = make_rays(rng, lo[pick], hi[pick], n_rays)
    pad = Q.ray_pad(o)
    enter, tn64, tf64 = exact_enter(o, d, lo[pick], hi[pick], pad.astype(np.float64) * 0.5)
    S, Bp, Bm = Q.make_qray(o, d, frame)
    tn, tf = Q.qnode_slabs(qlo[pick], qhi[pick], S, Bp, Bm, np.full(n_rays, np.inf, F))
    bad = enter & ~(tn <= tf)
    # a bound inside the exact segment (a hit there must not be culled); only where the segment is long against float32 rounding
    inside = enter & (tf64 - tn64 > 2.0 ** -16 * np.maximum(tn64, 1e-30)) & np.isfinite(tf64)
    tb = ((tn64 + tf64) * 0.5).astype(F)
    tn2, tf2 = Q.qnode_slabs(qlo[pick], qhi[pick], S, Bp, Bm, tb)
    bad |= inside & ~(tn2 <= tf2)
    return int(bad.sum()), int(enter.sum())


def test_a_forest_too_large_for_the_grid_keeps_the_float_nodes():
    """deep_chain reaches 3^39 ~ 4e18: its cell (~6e13) times the clamped 1 / d of an axis-parallel ray (1e18) times 2^23 overflows float32,
    and the plane arithmetic returns infinities.  Such a frame is never used (scene_prep.cpp requantize), not even with qnodes = 1."""
    frame, _ = Q.quantized_nodes(*tree("deep_chain"))
    assert frame[1, :3].max() > Q.MAX_CELL and not Q.in_use(frame, 1) and not Q.in_use(frame, -1)
    for name in SCENES:
        if name != "deep_chain":
            assert Q.in_use(Q.qframe(*tree(name)), 1), name


@pytest.mark.parametrize("name", [k for k in SCENES if k != "deep_chain"])
def test_slab_test_enters_every_box_the_exact_ray_enters(name):
    nodes, root = tree(name)
    for seed in range(4 if name in LOWER_FACE else 2):
        bad, checked = slab_failures(nodes, root, seed=seed)
        assert checked > 100_000
        assert bad == 0, f"{name} seed {seed}: {bad} of {checked} rays entering a float box are culled by its quantized box"


@pytest.mark.parametrize("name", LOWER_FACE)
def test_the_former_frame_culls_rays_the_float_box_takes(name):
    """Negative control for the slab test: on the frame before, rays near the lower faces are culled."""
    nodes, root = tree(name)
    bad = sum(slab_failures(nodes, root, Q.FORMER_GRID, seed=s)[0] for s in range(4))
    assert bad > 0


def test_restated_slab_test_matches_the_plane_formula():
    """make_qray + qnode_slabs place the plane of code q at (origin + q cell - (o +- pad)) / d to within one cell and 2^-20 relative."""
    rng = np.random.default_rng(7)
    n = 50_000
    frame = np.array([[-3.25, 0.5, 1e4, 0], [1e-3, 2e-5, 0.25, 0]], F)
    o = (rng.normal(size=(n, 3)) * 5).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    q = rng.integers(0, 65536, (n, 3))
    S, Bp, Bm = Q.make_qray(o, d, frame)
    t = Q.fma32((F(8388608.0) + q.astype(F)).astype(F), S, Bp).astype(np.float64)
    pad = Q.ray_pad(o).astype(np.float64)[:, None]
    exact = (frame[0, :3].astype(np.float64) + q * frame[1, :3].astype(np.float64) - (o.astype(np.float64) + pad)) / d.astype(np.float64)
    cell_t = frame[1, :3].astype(np.float64) / np.abs(d.astype(np.float64))
    assert (np.abs(t - exact) <= cell_t + 2.0 ** -20 * (np.abs(exact) + np.abs(frame[0, :3]) / np.abs(d))).all()
