"""A float64 model of WHERE things are, written from the geometry alone: a pinhole camera built from its pose, "where a hit point was"
from the identity of the primitive, and the checks tests/test_registration_model.py (the restatements) and
tests/test_gpu_registration.py (the kernels) run against it.

Every image-space kernel is held bit for bit to a numpy restatement of the same header text, so a misreading the two share (a half-pixel
offset, a swapped row order, a motion table applied backwards, a barycentric bound to the wrong vertex, an off-centre filter tap) agrees
on both sides.  Nothing here reads that text: no camera matrix, no motion table, no *_ref.py; of the package only what builds scenes
(handed in by the tests), and an object's localToWorldMatrix as data.  Conventions, as the reference's ray set-up has them: a left-handed camera that looks along +z, yaw about +y, positive pitch looks down, a vertical
field of view, row 0 at the bottom, and the centre of pixel (x, y) at (x, y).  A test helper, not a conftest."""
import numpy as np

DEFAULT_POSE = dict(position=(0.0, 1.0, -10.0), yaw_deg=0.0, pitch_deg=0.0, fov_deg=81.0)     # Scene1's camera


def pose(**kw):
    out = dict(DEFAULT_POSE)
    out.update(kw)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the camera ------------------------------------------------------------------------------------------------------------------------
def camera_axes(yaw_deg, pitch_deg):
    """(right, up, forward) in the world: the axes x, y, z turned by the pitch about x, then by the yaw about y (left-handed, so a
    positive yaw turns +z towards +x and a positive pitch turns +z towards -y)."""
    a, b = np.radians(yaw_deg), np.radians(pitch_deg)
    right = np.array([np.cos(a), 0.0, -np.sin(a)])
    up = np.array([np.sin(a) * np.sin(b), np.cos(b), np.cos(a) * np.sin(b)])
    forward = np.array([np.sin(a) * np.cos(b), -np.sin(b), np.cos(a) * np.cos(b)])
    return right, up, forward


def pinhole(P, W, H, position=DEFAULT_POSE["position"], yaw_deg=0.0, pitch_deg=0.0, fov_deg=81.0, aspect=None, at_infinity=False):
    """((qx, qy), depth) of world points P (..., 3) on a W x H image: the continuous pixel position (pixel centres at the integers, row
    0 at the bottom) and the distance along the viewing axis.  at_infinity: P holds directions, projected by the rotation alone.
    The image plane at depth 1 is 2 tan(fov / 2) tall and `aspect` (default W / H) times as wide; its lower left corner is the corner
    of pixel (0, 0), half a pixel before that pixel's centre."""
    P = np.asarray(P, np.float64)
    right, up, forward = camera_axes(yaw_deg, pitch_deg)
    v = P if at_infinity else P - np.asarray(position, np.float64)
    depth = v @ forward
    t = np.tan(np.radians(fov_deg) * 0.5)
    with np.errstate(all="ignore"):
        sx = (v @ right) / (depth * t * (W / H if aspect is None else aspect))   # -1 .. 1 across the image
        sy = (v @ up) / (depth * t)
        return ((sx + 1.0) * 0.5 * W - 0.5, (sy + 1.0) * 0.5 * H - 0.5), depth


def pixel_directions(W, H, yaw_deg=0.0, pitch_deg=0.0, fov_deg=81.0, aspect=None, **_):
    """(H, W, 3): the direction through the centre of every pixel (not normalised)."""
    right, up, forward = camera_axes(yaw_deg, pitch_deg)
    t = np.tan(np.radians(fov_deg) * 0.5)
    sx = ((np.arange(W) + 0.5) / W * 2.0 - 1.0)[None, :, None]
    sy = ((np.arange(H) + 0.5) / H * 2.0 - 1.0)[:, None, None]
    return forward + right * (sx * t * (W / H if aspect is None else aspect)) + up * (sy * t)


def pixel_grid(W, H):
    return np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))


def classes(hit, normal):
    """(surface, sky) of feature buffers: a hit with a finite positive distance, or kind 0."""
    k, z = np.asarray(normal)[..., 3], np.asarray(hit)[..., 3]
    sky = k == 0
    with np.errstate(invalid="ignore"):
        return ~sky & np.isfinite(z) & (z > 0) & np.isfinite(np.asarray(hit)[..., :3]).all(-1), sky


# ---- where a hit point was, from identity ---------------------------------------------------------------------------------------------------
class SceneData:
    """What identity needs of a scene state, as data: the MeshObjects' localToWorldMatrix (n, 16; column-major), _Vertices, _Indices,
    the spheres' centres and radii."""

    def __init__(self, scene=None, matrices=None, vertices=None, indices=None, centres=None, radii=None):
        if scene is not None:
            matrices = scene.mesh_objects["localToWorldMatrix"] if len(scene.mesh_objects) else np.zeros((0, 16))
            vertices, indices = scene.vertices, scene.indices
            centres = scene.spheres["position"] if len(scene.spheres) else np.zeros((0, 3))
            radii = scene.spheres["radius"] if len(scene.spheres) else np.zeros(0)
        self.matrices = np.array(matrices, np.float64).reshape(-1, 16)
        self.vertices = np.array(vertices, np.float64).reshape(-1, 3)
        self.indices = np.array(indices, np.int64).reshape(-1)
        self.centres = np.array(centres, np.float64).reshape(-1, 3)
        self.radii = np.array(radii, np.float64).reshape(-1)


def triangle_points(ids, data):
    """World points of triangle pixels from their identity: the id texel names the MeshObject (x), the slot of the triangle's first index
    (y, int bits) and the barycentrics u, v (z, w): the object-space point is A0 (1 - u - v) + A1 u + A2 v with A_r = vertices[indices[
    slot + r]], carried into the world by the object's matrix.  Texels that name no triangle give NaN."""
    ids = np.ascontiguousarray(ids, np.float32)
    o, slot = bits(ids[..., 0]), bits(ids[..., 1])
    u, v = ids[..., 2].astype(np.float64), ids[..., 3].astype(np.float64)
    ok = (o >= 0) & (o < len(data.matrices)) & (slot >= 0) & (slot <= len(data.indices) - 3)
    s = np.where(ok, slot, 0)
    A = [data.vertices[data.indices[s + r]] for r in range(3)] if len(data.indices) >= 3 else [np.zeros(ids.shape[:-1] + (3,))] * 3
    p = A[0] * (1.0 - u - v)[..., None] + A[1] * u[..., None] + A[2] * v[..., None]
    m = data.matrices[np.where(ok, o, 0)] if len(data.matrices) else np.zeros(ids.shape[:-1] + (16,))
    world = np.stack([m[..., c] * p[..., 0] + m[..., 4 + c] * p[..., 1] + m[..., 8 + c] * p[..., 2] + m[..., 12 + c] for c in range(3)], -1)
    return np.where(ok[..., None], world, np.nan)


def where_it_was(hit, normal, ids, now, then):
    """(H, W, 3): the world position, in the scene state `then`, of the surface point every pixel shows in the state `now` (SceneData):
    a triangle pixel through its triangle's previous vertices and previous matrix, a sphere pixel at prev_centre + (P - centre) r_prev / r
    (a sphere has no orientation to track), the ground plane where it is.  Sky and broken texels give NaN."""
    hit, normal = np.asarray(hit, np.float32), np.asarray(normal, np.float32)
    P = hit[..., :3].astype(np.float64)
    k, o = normal[..., 3], bits(np.ascontiguousarray(ids, np.float32)[..., 0])
    surface, _ = classes(hit, normal)
    out = np.where((surface & (k == 1))[..., None], P, np.nan)
    tri = surface & (k == 3)
    out = np.where(tri[..., None], triangle_points(ids, then), out)
    sph = surface & (k == 2) & (o >= 0) & (o < len(now.centres))
    if len(now.centres):
        oc = np.where(sph, o, 0)
        with np.errstate(all="ignore"):
            was = then.centres[oc] + (P - now.centres[oc]) * (then.radii[oc] / now.radii[oc])[..., None]
        out = np.where(sph[..., None], was, out)
    return out


def identity_residual(hit, normal, ids, now):
    """Largest |triangle_points(now) - hit.xyz| over the triangle pixels, in world units, and their number: the same construction with
    the current data must give back the hit point, which pins the u / v convention."""
    surface, _ = classes(hit, normal)
    tri = surface & (np.asarray(normal)[..., 3] == 3)
    d = np.abs(triangle_points(ids, now) - np.asarray(hit, np.float32)[..., :3].astype(np.float64)).max(-1)
    if not tri.any():
        return 0.0, 0
    return (float(d[tri].max()) if not np.isnan(d[tri]).any() else np.inf), int(tri.sum())


# ---- the checks -----------------------------------------------------------------------------------------------------------------------------
MARGIN = 1e-3                                                                # px: a pixel is checked where the model places it inside by more


def own_pixel_deviation(hit, normal, cam):
    """Check 1: the largest distance (px, per axis) between a surface pixel's own (x, y) and its hit point projected by the model."""
    H, W = hit.shape[:2]
    surface, _ = classes(hit, normal)
    (qx, qy), depth = pinhole(np.asarray(hit)[..., :3], W, H, **cam)
    X, Y = pixel_grid(W, H)
    d = np.maximum(np.abs(qx - X), np.abs(qy - Y))
    assert surface.any() and (depth[surface] > 0).all()
    return float(d[surface].max())


def model_positions(hit, normal, cam_then, cam_now, was=None):
    """(q (H, W, 2), depth, classed): where the model puts every classed pixel of the current view in the previous one.  Surface pixels:
    the point `was` (default: the hit point itself, a still scene) seen from cam_then; sky pixels: their own direction."""
    H, W = hit.shape[:2]
    surface, sky = classes(hit, normal)
    P = np.asarray(hit, np.float32)[..., :3].astype(np.float64) if was is None else was
    (sx, sy), sd = pinhole(P, W, H, **cam_then)
    (kx, ky), kd = pinhole(pixel_directions(W, H, **cam_now), W, H, at_infinity=True, **cam_then)
    q = np.stack([np.where(sky, kx, sx), np.where(sky, ky, sy)], -1)
    depth = np.where(sky, kd, sd)
    classed = (surface & np.isfinite(P).all(-1)) | sky
    return q, depth, classed


def window_masks(q, depth, classed):
    """(checked, outside): classed pixels the model places inside the window qx in (-1, W), qy in (-1, H) by more than MARGIN, in front
    of the camera; and those it places behind the camera or outside the window by more than MARGIN."""
    H, W = depth.shape
    with np.errstate(invalid="ignore"):
        front = depth > 0
        inside = (q[..., 0] > -1 + MARGIN) & (q[..., 0] < W - MARGIN) & (q[..., 1] > -1 + MARGIN) & (q[..., 1] < H - MARGIN)
        out = (q[..., 0] < -1 - MARGIN) | (q[..., 0] > W + MARGIN) | (q[..., 1] < -1 - MARGIN) | (q[..., 1] > H + MARGIN)
        behind = depth < 0
    return classed & front & inside, classed & (behind | (front & out))


def motion_deviation(out, q, depth, classed, only=None):
    """Check 2: (the largest |motion.xy + (x, y) - q| over the checked pixels in px, the number checked, the number of pixels the model
    puts outside the previous view, how many of THOSE hold anything but zeros in colour, count or motion).  only: a mask to stay in."""
    H, W = depth.shape
    checked, outside = window_masks(q, depth, classed)
    if only is not None:
        checked, outside = checked & only, outside & only
    X, Y = pixel_grid(W, H)
    m = np.asarray(out["motion"], np.float64)
    d = np.maximum(np.abs(m[..., 0] + X - q[..., 0]), np.abs(m[..., 1] + Y - q[..., 1]))
    nonzero = (np.asarray(out["color"]) != 0).any(-1) | (np.asarray(out["count"]) != 0).any(-1) | (np.asarray(out["motion"]) != 0).any(-1)
    return (float(d[checked].max()) if checked.any() else 0.0), int(checked.sum()), int(outside.sum()), int((nonzero & outside).sum())


def ramp_history(W, H):
    """Check 3's history: prev_color = (x, y, x + y, 1), prev_count.x = 1 + x (float32, exact)."""
    X, Y = pixel_grid(W, H)
    color = np.stack([X, Y, X + Y, np.ones_like(X)], -1).astype(np.float32)
    count = np.zeros((H, W, 4), np.float32)
    count[..., 0] = 1.0 + X
    return color, count


def gather_deviation(out, q, depth, classed, of=None):
    """Check 3: with the ramp history and max_history 0, a pixel whose taps are valid (motion.z = S >= 0.999) must hold the ramp at the
    model's q, since bilinear interpolation reproduces a ramp exactly.  (the largest deviation of colour (qx, qy, qx + qy, 1) and count
    1 + qx, the share of the pixels of `of` that were so checked).
    S >= 0.999 also lets through a pixel that lost a tap of weight 1 - S <= 0.001; the renormalised sum of the other three is then off
    by at most (1 - S) times the ramp's span over the footprint, which is 2 (the x + y channel).  That known amount, 2 (1 - S), is taken
    off such a pixel's deviation; with all four taps 1 - S is a rounding error (<= 3e-7) and nothing is taken off."""
    checked, _ = window_masks(q, depth, classed)
    S = np.asarray(out["motion"], np.float64)[..., 2]
    sel = checked & (S >= 0.999)
    if of is not None:
        sel = sel & of
    want = np.stack([q[..., 0], q[..., 1], q[..., 0] + q[..., 1], np.ones_like(depth)], -1)
    d = np.abs(np.asarray(out["color"], np.float64) - want).max(-1)
    d = np.maximum(d, np.abs(np.asarray(out["count"], np.float64)[..., 0] - (1.0 + q[..., 0])))
    d = np.maximum(d - 2.0 * np.maximum(1.0 - S, 0.0), 0.0)
    base = of if of is not None else classed
    return (float(d[sel].max()) if sel.any() else np.inf), float(sel.sum() / max(int(base.sum()), 1))


# ---- upsampling --------------------------------------------------------------------------------------------------------------------------------
def low_position(n_full, n_low):
    """Where the centre of full-grid pixel X lies on a low grid over the same image: both grids span it from edge to edge, so the
    normalised position (X + 0.5) / n_full equals (q + 0.5) / n_low."""
    return (np.arange(n_full) + 0.5) * n_low / n_full - 0.5


def screen_ramp(w, h):
    """((x + 0.5) / w, (y + 0.5) / h, their sum, 1): a colour that is the texel centre's normalised screen position."""
    X, Y = pixel_grid(w, h)
    sx, sy = (X + 0.5) / w, (Y + 0.5) / h
    return np.stack([sx, sy, sx + sy, np.ones_like(sx)], -1).astype(np.float32)


def seen_ramp(low_hit, low_normal, cam):
    """screen_ramp as the low grid's texels SEE it: a surface texel takes the normalised screen position of its own hit point under the
    model (on a grid rendered where it should be, that is its centre); a sky texel keeps its centre's."""
    h, w = low_hit.shape[:2]
    surface, _ = classes(low_hit, low_normal)
    (qx, qy), _ = pinhole(np.asarray(low_hit)[..., :3], w, h, **cam)
    X, Y = pixel_grid(w, h)
    sx, sy = (np.where(surface, qx, X) + 0.5) / w, (np.where(surface, qy, Y) + 0.5) / h
    return np.stack([sx, sy, sx + sy, np.ones_like(sx)], -1).astype(np.float32)


def four_taps_inside(w, h, W, H):
    """(H, W) bool: the full-grid pixels whose bilinear footprint on the low grid lies inside it (a tap of weight 0 does not count)."""
    qx, qy = low_position(W, w), low_position(H, h)
    return ((qy >= 0) & (qy <= h - 1))[:, None] & ((qx >= 0) & (qx <= w - 1))[None, :]


def upsample_deviation(color, W, H):
    """(H, W): the largest deviation per pixel of an upsampled screen_ramp from the full grid's own ((X + 0.5) / W, (Y + 0.5) / H, sum, 1)."""
    return np.abs(np.asarray(color, np.float64) - screen_ramp(W, H).astype(np.float64)).max(-1)


def grid_relation_deviation(hit, normal, w, h, cam, qx, qy):
    """Check 5c: full-grid hit points projected by the model at the LOW size against the kernel's position on the low grid (qx (W,), qy
    (H,)), in low pixels, over the surface pixels."""
    surface, _ = classes(hit, normal)
    (mx, my), _ = pinhole(np.asarray(hit)[..., :3], w, h, **cam)
    d = np.maximum(np.abs(mx - np.asarray(qx, np.float64)[None, :]), np.abs(my - np.asarray(qy, np.float64)[:, None]))
    return float(d[surface].max())


# ---- denoiser and bloom --------------------------------------------------------------------------------------------------------------------------
def uniform_guides(W, H, depth=7.0):
    """(hit, normal) of one plane seen at a constant depth with a constant normal (kind 1): no edge-stopping term can tell two pixels
    apart, so a symmetric filter must return a ramp unchanged."""
    hit = np.zeros((H, W, 4), np.float32)
    hit[..., 3] = depth
    normal = np.zeros((H, W, 4), np.float32)
    normal[..., 1], normal[..., 3] = 1.0, 1.0
    return hit, normal


def denoise_ramp(W, H):
    X, Y = pixel_grid(W, H)
    return np.stack([X, Y, 0.25 * X - 0.5 * Y + 40.0, np.ones_like(X)], -1).astype(np.float32)


def interior(W, H, border):
    """(H, W) bool: pixels farther than `border` from every edge."""
    X, Y = pixel_grid(W, H)
    return (X > border) & (X < W - 1 - border) & (Y > border) & (Y < H - 1 - border)


def impulse(W, H, x, y, value=(3.0, 2.0, 1.5)):
    src = np.zeros((H, W, 4), np.float32)
    src[..., 3] = 1.0
    src[y, x, :3] = value
    return src


def glow_moments(dst, src):
    """Per colour channel: (centroid x, centroid y, sum) of dst - src, in float64; and the largest |dst - src| within two pixels of a border."""
    g = np.asarray(dst, np.float64)[..., :3] - np.asarray(src, np.float64)[..., :3]
    H, W = g.shape[:2]
    X, Y = pixel_grid(W, H)
    s = g.sum((0, 1))
    cx = (g * X[..., None]).sum((0, 1)) / s
    cy = (g * Y[..., None]).sum((0, 1)) / s
    edge = ~interior(W, H, 1)
    return cx, cy, s, float(np.abs(g[edge]).max())


# ---- the cases both test files share (scene states as data; the matrices handed to the code under test come from the package) ------------------
SIZES = [(67, 45), (96, 64)]
POSE_A = pose()
POSE_B = pose(position=(0.35, 1.2, -9.6), yaw_deg=4.0)
POSE_BEHIND = pose(position=(0.0, 1.0, 4.0))                                  # as the previous camera: most of the scene lies behind it
STATIC_PAIRS = {"move": (POSE_A, POSE_B), "behind": (POSE_BEHIND, POSE_A)}
# the default camera sees the meshes a few pixels tall; the moved and the deformed objects are looked at from nearby
MOVED_A = pose(position=(2.4, 1.4, -7.0))                                     # in front of the icosphere and sphere 0
MOVED_B = pose(position=(2.5, 1.45, -7.1), yaw_deg=1.0)
DEFORM_A = pose(position=(-3.5, 1.2, -3.0))                                   # in front of the blob
DEFORM_B = pose(position=(-3.4, 1.25, -3.1), yaw_deg=1.5)
PLANE_POSE = pose(position=(0.0, 2.5, -9.5), pitch_deg=75.0)                  # looks down in front of the objects (the view ends at z = -5.9): ground only
# The moved mesh is the icosphere, not the blob: the blob's matrix scales unevenly and its shading normals, carried by the matrix's
# linear part, stand up to 70 degrees off its faces, so the plane test of a moved pixel (which uses them) leaves only 0.42 of its
# footprints whole at 67 x 45, whatever the blob's tessellation.  That is the scene's doing, not registration's; the deformed path, which
# uses face normals, takes the blob.
MOVED_MESH, MOVED_SPHERE, DEFORMED_MESH = 1, 0, 0
UPSAMPLE_PAIRS = [(33, 22, 66, 44), (23, 25, 67, 45), (67, 45, 67, 45)]       # ratio 2, a non-integer ratio, ratio 1
MIXED_PAIRS = [(23, 25, 67, 45), (48, 32, 96, 64)]


def camera_of(scenes, W, H, cam):
    """(_CameraToWorld, _CameraInverseProjection) of a pose, as the package makes them (16 floats each).  A pose with an "aspect" keeps
    that width : height of the view on a grid of another shape (a low grid under the full grid's camera)."""
    cam = dict(cam)
    aspect = cam.pop("aspect", None)
    return scenes.camera_matrices(W, H, **cam) if aspect is None else scenes.camera_matrices(aspect, 1.0, **cam)


def posed(scenes, sc, cam):
    """A copy of scene `sc` seen from the pose `cam`."""
    import copy
    s = copy.copy(sc)
    s.camera_to_world, s.camera_inverse_projection = camera_of(scenes, sc.width, sc.height, cam)
    return s


def moved_scene(scenes, sc):
    """A copy of the mixed scene with MeshObject 1 (the icosphere) turned by 10 degrees about its own origin, grown by 8 % and shifted,
    and sphere 0 shifted and grown by 10 %; object-level heaps rebuilt."""
    import copy
    s = copy.copy(sc)
    mo, sp = sc.mesh_objects.copy(), sc.spheres.copy()
    m = np.asarray(mo[MOVED_MESH]["localToWorldMatrix"], np.float64).reshape(4, 4).T
    a = np.radians(10.0)
    new = m.copy()
    new[:3, :3] = (np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) * 1.08) @ m[:3, :3]
    new[:3, 3] = m[:3, 3] + (0.22, 0.06, -0.1)
    mo[MOVED_MESH]["localToWorldMatrix"] = new.T.reshape(16).astype(np.float32)
    sp[MOVED_SPHERE]["position"] = sp[MOVED_SPHERE]["position"] + np.array([0.07, 0.02, -0.05], np.float32)
    sp[MOVED_SPHERE]["radius"] = np.float32(1.1) * sp[MOVED_SPHERE]["radius"]
    s.mesh_objects, s.spheres = mo, sp
    s.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(mo, s.vertices, s.indices))
    s.sphere_bvh = scenes.build_object_bvh(*scenes.sphere_bounds(sp))
    return s


def deformed_positions(sc):
    """The blob's object-space vertices displaced by a smooth known field: along the radius by 12 % sin(3 x + 1) cos(2 y), and sheared
    along x by 0.12 sin(2 y)."""
    n = len(np.unique(sc.indices[int(sc.mesh_objects[DEFORMED_MESH]["indices_offset"]):][: int(sc.mesh_objects[DEFORMED_MESH]["indices_count"])]))
    v = np.asarray(sc.vertices[:n], np.float64)
    out = v * (1.0 + 0.12 * np.sin(3.0 * v[:, :1] + 1.0) * np.cos(2.0 * v[:, 1:2]))
    out[:, 0] += 0.12 * np.sin(2.0 * v[:, 1])
    return out.astype(np.float32)


def deformed_scene(scenes, sc):
    """A copy of the mixed scene with the blob (MeshObject 0, whose vertices come first) deformed; normals and heap rebuilt."""
    import copy
    s = copy.copy(sc)
    new = deformed_positions(sc)
    v = np.array(sc.vertices, np.float32)
    v[: len(new)] = new
    s.vertices = v
    s.normals = scenes.compute_normals(s.vertices, s.indices)
    s.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(s.mesh_objects, s.vertices, s.indices))
    return s


def inverted_table(table):
    """A motion table (n, 12: the linear part column by column, then the translation) with every entry inverted: the wrong direction."""
    out = np.array(table, np.float32)
    for e in out:
        a = np.asarray(e[:9], np.float64).reshape(3, 3).T
        ia = np.linalg.inv(a)
        e[:9], e[9:] = ia.T.reshape(9), -ia @ np.asarray(e[9:], np.float64)
    return out


def half_pixel_off(invp16, w, h):
    """A _CameraInverseProjection whose pixel-centre rays pass half a pixel further along x and y: what a renderer that put the centre
    of pixel (x, y) at (x + 0.5, y + 0.5) would trace."""
    m = np.asarray(invp16, np.float64).reshape(4, 4).T
    shift = np.eye(4)
    shift[0, 3], shift[1, 3] = 1.0 / w, 1.0 / h
    return np.ascontiguousarray((m @ shift).T.astype(np.float32).reshape(16))
