"""The camera rays and the material table of include/urt.h urt_render_aov, restated in numpy with the normative float32 arithmetic, and
the whole call composed from them and the oracle (tests/test_gpu_aov.py, tests/command_stream.py).  No GPU needed."""
import numpy as np

from oracle import pyoracle

F = np.float32


# ---- fma32 / dot32 as in test_gpu_ray_query.py ---------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma (urt_math.h f_fma) in numpy: the float64 product is exact; the sum is rounded to odd in float64 (TwoSum error term)
    and then to float32, which rounds the exact a * b + c correctly."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    odd = (err != 0) & ((s.view(np.uint64) & 1) == 0)
    s = np.where(odd, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def dot32(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(F)))


def mul_m4(m, x, y, z, w):
    """urt_math.h mul_m4: mul(M, float4(x, y, z, w)).xyz, M in Unity's column-major order, one fma chain per row."""
    m = np.asarray(m, F)
    x, y, z, w = (np.broadcast_to(np.asarray(q, F), np.shape(x)) for q in (x, y, z, w))
    return np.stack([fma32(m[12 + r], w, fma32(m[8 + r], z, fma32(m[4 + r], y, (m[r] * x).astype(F)))) for r in range(3)], axis=-1)


def normalize32(a):
    inv = (F(1) / np.sqrt(dot32(a, a))).astype(F)
    return (a * inv[..., None]).astype(F)


def camera_rays(sc, w, h, frame=None):
    """CreateCameraRay (RS:142-153) of every pixel, (h, w, 3) origins and directions.  frame = None: the pixel centre; (pixel_offset_x,
    pixel_offset_y, seed): the first sample's uv of RS:448-449 with the two rand() draws."""
    X, Y = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    if frame is None:
        u = ((X + F(0.5)) / F(w) * F(2) - F(1)).astype(F)
        v = ((Y + F(0.5)) / F(h) * F(2) - F(1)).astype(F)
    else:
        pox, poy, seed = (F(q) for q in frame)
        s0 = np.full(X.shape, seed, F)
        r0 = pyoracle.math_probe("rand", s0, X, Y)
        r1 = pyoracle.math_probe("rand", (s0 + F(0.5)).astype(F), X, Y)
        u = ((X + r0 + pox) / F(w) * F(2) - F(1)).astype(F)
        v = ((Y + r1 + poy) / F(h) * F(2) - F(1)).astype(F)
    c2w, invp = np.asarray(sc.camera_to_world, F), np.asarray(sc.camera_inverse_projection, F)
    zero = np.zeros(X.shape, F)
    o = mul_m4(c2w, zero, zero, zero, F(1))
    d = mul_m4(invp, u, v, zero, F(1))
    d = mul_m4(c2w, d[..., 0], d[..., 1], d[..., 2], zero)
    return o, normalize32(d)


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def material_albedo(sc):
    """(n_spheres + n_meshes + 1, 4): min(1 - specular, albedo) in float32 and smoothness, in the library's material order."""
    lights = [sc.spheres["lighting"][i] for i in range(len(sc.spheres))] + [sc.mesh_objects["lighting"][i] for i in range(len(sc.mesh_objects))]
    out = np.zeros((len(lights) + 1, 4), F)
    for k, l in enumerate(lights):
        out[k, :3] = np.minimum((F(1) - l["color_specular"].astype(F)).astype(F), l["color_albedo"].astype(F))
        out[k, 3] = l["smoothness"]
    out[-1, :3] = np.minimum(F(1) - np.zeros(3, F), np.array([0.5, 0.3, 0.15], F))
    out[-1, 3] = F(0.3)
    return out


def material_index(sc, kind, obj):
    ns, nm = len(sc.spheres), len(sc.mesh_objects)
    return np.where(kind == 1, ns + nm, np.where(kind == 2, obj, ns + obj))


def render_aov_ref(sc, frame=None, mode=0):
    """(hit, normal, albedo, id) images (h, w, 4) float32 of urt_render_aov for scene `sc` (its camera, sky and size): the rays of
    camera_rays (frame as there), traced and shaded by the oracle (pyoracle.Oracle.aov).  id.xy hold int32 bits."""
    O, D = camera_rays(sc, sc.width, sc.height, frame)
    return pyoracle.Oracle(sc).aov(np.broadcast_to(O, D.shape), D, mode)
