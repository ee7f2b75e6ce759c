"""CPU: per-object motion for the temporal reprojection (include/urt.h urt_reproject_objects, urt_host_mesh_motion,
urt_host_sphere_motion) — the header compiles as C99 and its two structs have one layout in gcc and ctypes, the symbols are exported and
declared in the C# binding, a NULL context is rejected without a device, the Python wrapper validates before it calls the library, the
host helpers agree with numpy.linalg, and the float32 restatement (tests/reproject_motion_ref.py) removes the two defects of plain
reprojection on analytic scenes: an in-plane move that slides the image over the surface, and a move across the plane test that loses
the history."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from reproject_motion_ref import IDENTITY, apply_motion, reproject_objects_ref
from reproject_ref import analytic_aovs, reproject_ref
from unityraytracer_amd import _lib, host_scene, scenes, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
IMAGE_FIELDS = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color", "count", "motion")
MOTION_FIELDS = ("mesh_motion", "sphere_motion", "moved_max_history", "flags")


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(urt_ReprojectMotion, {f})" for f in MOTION_FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int (*fn)(urt_context*, const urt_ReprojectImages*, const urt_ReprojectParams*, const urt_ReprojectMotion*) = urt_reproject_objects;\n'
                   'int (*fm)(const void*, const void*, int, urt_ObjectMotion*) = urt_host_mesh_motion;\n'
                   'int (*fs)(const void*, const void*, int, urt_ObjectMotion*) = urt_host_sphere_motion;\n'
                   'int main(void) {\n'
                   f'  size_t p[] = {{sizeof(urt_ObjectMotion), offsetof(urt_ObjectMotion, a), sizeof(urt_ReprojectMotion), {offs}, URT_STRIDE_OBJECTMOTION}};\n'
                   '  for (unsigned k = 0; k < sizeof p / sizeof p[0]; k++) printf("%zu ", p[k]);\n'
                   '  return fn == 0 || fm == 0 || fs == 0;\n}\n')
    subprocess.run(["gcc", *inc, "-c", str(src), "-o", str(tmp_path / "layout.o")], check=True)     # compiles (linking needs the library)
    src2 = tmp_path / "sizes.c"
    src2.write_text(src.read_text().replace("= urt_reproject_objects", "= 0").replace("= urt_host_mesh_motion", "= 0")
                    .replace("= urt_host_sphere_motion", "= 0").replace("return fn == 0 || fm == 0 || fs == 0;", "return fn != 0 || fm != 0 || fs != 0;"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", *inc, str(src2), "-o", str(exe)], check=True)
    p = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert p[0] == C.sizeof(_lib.ObjectMotion) == 48 and p[1] == _lib.ObjectMotion.a.offset == 0
    assert p[2] == C.sizeof(_lib.ReprojectMotion) == 24
    assert p[3:7] == [getattr(_lib.ReprojectMotion, f).offset for f in MOTION_FIELDS] == [0, 8, 16, 20]
    assert p[7] == 48


def test_symbols_are_declared_exported_and_in_the_csharp_binding(built_library):
    names = ("urt_reproject_objects", "urt_host_mesh_motion", "urt_host_sphere_motion")
    text = open(os.path.join(ROOT, "include", "urt.h")).read()
    assert re.search(r"URT_API int urt_reproject_objects\(urt_context\* ctx, const urt_ReprojectImages\* images, const urt_ReprojectParams\* params,"
                     r"\s*const urt_ReprojectMotion\* motion\);", text)
    assert "Moving objects have no motion vectors" not in text
    lib = C.CDLL(built_library)
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    for n in names:
        assert n in _lib.ABI_SYMBOLS and hasattr(lib, n), n
        assert re.search(rf"\[DllImport\(Lib\)\]\s+internal static extern int {n}\(", cs), n
    m = re.search(r"internal struct ReprojectMotion \{(.*?)\n    \}", cs, re.S)
    assert m and re.findall(r"public (ulong|float|int) ([\w, ]+);", m.group(1)) == [("ulong", "meshMotion, sphereMotion"), ("float", "movedMaxHistory"),
                                                                                   ("int", "flags")]
    assert "public static void MoveObjects<" in shim and "urt_reproject_objects(ctx, in im, in p, in mo)" in shim
    assert _lib.load().urt_abi_version() == 4


def test_null_context_and_bad_host_arguments_are_rejected(built_library):
    lib = _lib.load()
    im, p, mo = _lib.ReprojectImages(*range(1, 12)), _lib.ReprojectParams(), _lib.ReprojectMotion()
    assert lib.urt_reproject_objects(None, C.byref(im), C.byref(p), C.byref(mo)) == 1       # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_reproject_objects(None, C.byref(im), C.byref(p), None) == 1
    out = np.zeros((2, 12), F)
    objs = np.zeros(2, scenes.MESHOBJECT_DT)
    for fn in (lib.urt_host_mesh_motion, lib.urt_host_sphere_motion):
        assert fn(None, None, 0, None) == 0                                                # nothing to do
        assert fn(objs.ctypes.data, objs.ctypes.data, -1, out.ctypes.data) == 1
        assert b"negative" in lib.urt_host_last_error()
        assert fn(None, objs.ctypes.data, 2, out.ctypes.data) == 1
        assert fn(objs.ctypes.data, None, 2, out.ctypes.data) == 1
        assert fn(objs.ctypes.data, objs.ctypes.data, 2, None) == 1
        assert b"NULL" in lib.urt_host_last_error()
    with pytest.raises(ValueError):
        host_scene.mesh_motion(objs, objs[:1])


# ---- 2. the Python wrapper, on a stub library ---------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_reproject(self, *a):
        self.calls.append(("reproject",))
        return 0

    def urt_reproject_objects(self, ctx, im, p, mo):
        m = mo._obj
        self.calls.append(("reproject_objects", m.mesh_motion, m.sphere_motion, m.moved_max_history, m.flags))
        return 0


def stub_context():
    ctx = object.__new__(unity_api.Context)
    ctx.lib = _StubLib()
    ctx._h = C.c_void_p(1)
    ctx.device = 0
    return ctx


def stub_texture(ctx, handle, w=4, h=3):
    t = object.__new__(unity_api.RenderTexture)
    t.ctx, t.handle, t.width, t.height = ctx, handle, w, h
    return t


def stub_buffer(ctx, handle, count=3, stride=48):
    b = object.__new__(unity_api.ComputeBuffer)
    b.ctx, b.handle, b.count, b.stride = ctx, handle, count, stride
    return b


def reproject_kwargs(ctx):
    kw = {n: stub_texture(ctx, 11 + k) for k, n in enumerate(IMAGE_FIELDS)}
    kw["prev_world_to_clip"] = np.eye(4, dtype=F).reshape(16)
    return kw


MOTION_BAD = {
    "mesh_motion_array": (TypeError, lambda c: {"mesh_motion": np.zeros((2, 12), F)}),
    "sphere_motion_int": (TypeError, lambda c: {"sphere_motion": 5}),
    "mesh_motion_other_context": (ValueError, lambda c: {"mesh_motion": stub_buffer(stub_context(), 70)}),
    "sphere_motion_released": (ValueError, lambda c: {"sphere_motion": stub_buffer(c, 0)}),         # the unknown handle of the ABI
    "mesh_motion_stride": (ValueError, lambda c: {"mesh_motion": stub_buffer(c, 71, stride=64)}),
    "sphere_motion_stride": (ValueError, lambda c: {"sphere_motion": stub_buffer(c, 72, stride=12)}),
    "moved_max_history_nan": (ValueError, lambda c: {"moved_max_history": float("nan")}),
    "moved_max_history_negative": (ValueError, lambda c: {"moved_max_history": -2.0}),
    "moved_max_history_half": (ValueError, lambda c: {"moved_max_history": 0.5}),
    "moved_max_history_str": (TypeError, lambda c: {"moved_max_history": "4"}),
}


@pytest.mark.parametrize("case", sorted(MOTION_BAD))
def test_wrapper_rejects_bad_motion_arguments_before_the_library(case):
    exc, change = MOTION_BAD[case]
    ctx = stub_context()
    with pytest.raises(exc):
        ctx.reproject(**reproject_kwargs(ctx), **change(ctx))
    assert ctx.lib.calls == []


def test_wrapper_calls_plain_reproject_without_tables_and_the_new_entry_with_them():
    ctx = stub_context()
    ctx.reproject(**reproject_kwargs(ctx))
    ctx.reproject(**reproject_kwargs(ctx), mesh_motion=None, sphere_motion=None, moved_max_history=0)
    ctx.reproject(**reproject_kwargs(ctx), mesh_motion=stub_buffer(ctx, 70))
    ctx.reproject(**reproject_kwargs(ctx), sphere_motion=stub_buffer(ctx, 71), moved_max_history=8)
    ctx.reproject(**reproject_kwargs(ctx), mesh_motion=stub_buffer(ctx, 70), sphere_motion=stub_buffer(ctx, 71), moved_max_history=1.0)
    ctx.reproject(**reproject_kwargs(ctx), moved_max_history=4.0)
    assert ctx.lib.calls == [("reproject",), ("reproject",), ("reproject_objects", 70, 0, 0.0, 0), ("reproject_objects", 0, 71, 8.0, 0),
                             ("reproject_objects", 70, 71, 1.0, 0), ("reproject_objects", 0, 0, 4.0, 0)]
    with pytest.raises(TypeError):
        ctx.reproject(*reproject_kwargs(ctx).values(), None, 64.0, 0.9, 0.02, stub_buffer(ctx, 70))     # the additions are keyword-only
    for bad in (np.zeros((2, 11), F), np.zeros(12, F), np.zeros((0, 12), F)):
        with pytest.raises(ValueError):
            ctx.reproject_arrays(*[np.zeros((3, 4, 4), F)] * 8, np.eye(4).reshape(16), np.eye(4).reshape(16), np.eye(4).reshape(16), mesh_motion=bad)


# ---- 3. the host helpers -----------------------------------------------------------------------------------------------------------------
def random_pose(rng, scale_range=(0.3, 3.0)):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    s = float(rng.uniform(*scale_range))
    return scenes.trs_quat(tuple(rng.uniform(-5, 5, 3)), tuple(q), (s, s, s))


def mesh_objects_of(mats):
    mo = np.zeros(len(mats), scenes.MESHOBJECT_DT)
    for k, m in enumerate(mats):
        mo[k]["localToWorldMatrix"] = m
    return mo


def test_mesh_motion_agrees_with_numpy_linalg(built_library):
    """The helper inverts curL by cofactors, numpy.linalg by LU with pivoting: both in float64, but not the same operations, so the two
    float64 results differ in their last bits.  After the one rounding to float32 most entries are equal bit for bit; an entry may
    differ by one float32 ulp AT THE MAGNITUDE OF THE TERMS IT SUMS (s below) when the float64 values straddle a rounding boundary, or
    when cancellation leaves 0 on one path and 1e-17 on the other.  Nothing larger is accepted."""
    rng = np.random.default_rng(11)
    n = 200
    prev, cur = [random_pose(rng) for _ in range(n)], [random_pose(rng) for _ in range(n)]
    got = host_scene.mesh_motion(mesh_objects_of(prev), mesh_objects_of(cur))
    equal = 0
    for k in range(n):
        Lp, Lc = (np.asarray(m, np.float64).reshape(4, 4).T for m in (prev[k], cur[k]))
        inv = np.linalg.inv(Lc)
        A = (Lp @ inv)[:3]
        ref = np.concatenate([A[:, :3].T.reshape(9), A[:, 3]]).astype(F)
        s_lin = np.abs(Lp[:3, :3]).max() * np.abs(inv[:3, :3]).max()
        s_t = max(np.abs(Lp[:3, 3]).max(), np.abs(A[:, :3]).max() * np.abs(Lc[:3, 3]).max())
        tol = np.concatenate([np.full(9, np.spacing(F(s_lin))), np.full(3, np.spacing(F(s_t)))])
        tol = np.maximum(tol, np.spacing(np.abs(ref)))
        assert (np.abs(got[k].astype(np.float64) - ref.astype(np.float64)) <= tol).all(), (k, got[k], ref)
        equal += int((got[k].view(np.uint32) == ref.view(np.uint32)).all())
    assert equal >= n // 2, equal                                         # bit-equal is the rule, a last-place difference the exception


def test_motion_entries_take_current_points_to_previous_ones(built_library):
    """entry(curL * p) == prevL * p within float32 rounding: twelve rounded entries, a rounded point, and three products and three sums
    per row, each with relative error 2^-24 of the terms' magnitudes; 16 of them bound the row generously."""
    rng = np.random.default_rng(12)
    prev, cur = [random_pose(rng) for _ in range(50)], [random_pose(rng) for _ in range(50)]
    tab = host_scene.mesh_motion(mesh_objects_of(prev), mesh_objects_of(cur))
    p = rng.uniform(-1, 1, (64, 3))
    for k in range(50):
        Lp, Lc = (np.asarray(m, np.float64).reshape(4, 4).T for m in (prev[k], cur[k]))
        wc = (p @ Lc[:3, :3].T + Lc[:3, 3]).astype(F)
        want = p @ Lp[:3, :3].T + Lp[:3, 3]
        got = apply_motion(tab[k], wc).astype(np.float64)
        a = np.abs(tab[k].astype(np.float64))
        mag = np.stack([a[r] * np.abs(wc[:, 0]) + a[3 + r] * np.abs(wc[:, 1]) + a[6 + r] * np.abs(wc[:, 2]) + a[9 + r] for r in range(3)], -1)
        assert (np.abs(got - want) <= 16 * 2.0 ** -24 * mag).all(), k
    sp_a, sp_b = scenes.make_spheres(20, 5.0, seed=3), scenes.make_spheres(20, 5.0, seed=4)
    st = host_scene.sphere_motion(sp_a, sp_b)
    for k in range(20):
        s = float(sp_a[k]["radius"]) / float(sp_b[k]["radius"])
        ref = np.zeros(12)
        ref[[0, 4, 8]] = s
        ref[9:] = sp_a[k]["position"].astype(np.float64) - s * sp_b[k]["position"].astype(np.float64)
        assert st[k].tobytes() == ref.astype(F).tobytes(), k                  # the same float64 operations: equal bit for bit
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        on_b = (sp_b[k]["position"] + sp_b[k]["radius"] * d).astype(F)
        on_a = sp_a[k]["position"].astype(np.float64) + float(sp_a[k]["radius"]) * d
        assert np.abs(apply_motion(st[k], on_b) - on_a).max() <= 1e-5


def test_identity_bits_for_equal_inputs_and_nan_for_singular_ones(built_library):
    rng = np.random.default_rng(13)
    mats = [random_pose(rng) for _ in range(4)]
    mo = mesh_objects_of(mats)
    cur = mo.copy()
    cur[1]["localToWorldMatrix"] = random_pose(rng)
    cur[2]["localToWorldMatrix"] = scenes.trs(translate=(1, 2, 3), scale=(1.0, 0.0, 1.0))      # singular
    cur[3]["lighting"]["smoothness"] = 0.5                                                     # a material change is not a move
    t = host_scene.mesh_motion(mo, cur)
    assert t[0].tobytes() == IDENTITY.tobytes() and t[3].tobytes() == IDENTITY.tobytes()
    assert t[1].tobytes() != IDENTITY.tobytes() and np.isfinite(t[1]).all()
    assert np.isnan(t[2]).all()
    back = host_scene.mesh_motion(cur, mo)                                                      # a singular PREVIOUS matrix is no problem
    assert np.isfinite(back[2]).all()
    sp = scenes.make_spheres(4, 5.0, seed=5)
    cs = sp.copy()
    cs[1]["position"] += F(0.25)
    cs[2]["radius"] = 0.0
    cs[3]["lighting"]["smoothness"] = 0.25
    t = host_scene.sphere_motion(sp, cs)
    assert t[0].tobytes() == IDENTITY.tobytes() and t[3].tobytes() == IDENTITY.tobytes()
    assert t[1].tobytes() != IDENTITY.tobytes() and np.isnan(t[2]).all()
    cs[2]["radius"] = -1.0
    assert np.isnan(host_scene.sphere_motion(sp, cs)[2]).all()


# ---- 4. the reference on analytic scenes -------------------------------------------------------------------------------------------------
W, H = 160, 120
WALL = ("wall", 6.0, (-4.0, 4.0), (0.0, 3.0), 2)          # MeshObject 2
SPHERE = ("sphere", (-0.5, 1.0, 1.0), 1.0, 1)             # sphere 1


def translation(dx=0.0, dy=0.0, dz=0.0):
    t = IDENTITY.copy()
    t[9:] = (dx, dy, dz)
    return t


def table(n, **entries):
    t = np.tile(IDENTITY, (n, 1))
    for k, e in entries.items():
        t[int(k[1:])] = e
    return t


def erode(mask, n):
    m = mask.copy()
    for _ in range(n):
        e = m.copy()
        e[1:] &= m[:-1]; e[:-1] &= m[1:]; e[:, 1:] &= m[:, :-1]; e[:, :-1] &= m[:, 1:]
        e[0] = e[-1] = False
        e[:, 0] = e[:, -1] = False
        m = e
    return m


def history(seed=0, count=16.0):
    """A history whose red channel is the pixel's x index (so a shift is visible), with a uniform count."""
    color = np.random.default_rng(seed).uniform(0.1, 1.0, (H, W, 4)).astype(F)
    color[..., 0] = np.arange(W, dtype=F)[None, :]
    cnt = np.zeros((H, W, 4), F)
    cnt[..., 0] = count
    return color, cnt


def case(prev_objects, cur_objects):
    cam = scenes.camera_matrices(W, H)
    return cam, analytic_aovs(W, H, *cam, objects=prev_objects), analytic_aovs(W, H, *cam, objects=cur_objects), scenes.world_to_clip(*cam)


def pixel_width_at(cam, z):
    """The world-space width of one pixel on the plane z = const in front of the (unrotated) camera."""
    c2w, invp = (np.asarray(m, np.float64).reshape(4, 4).T for m in cam)
    xs = []
    for px in (0, 1):
        e = invp @ np.array([(px + 0.5) / W * 2 - 1, 0.0, 0.0, 1.0])
        d = c2w[:3, :3] @ e[:3]
        xs.append(c2w[0, 3] + (z - c2w[2, 3]) * d[0] / d[2])
    return xs[1] - xs[0]


def test_in_plane_move_keeps_the_history_shifted_where_plain_reprojection_slides_it():
    cam = scenes.camera_matrices(W, H)
    dx = pixel_width_at(cam, WALL[1])
    moved_wall = ("wall", WALL[1], (WALL[2][0] + dx, WALL[2][1] + dx), WALL[3], WALL[4])
    cam, prev, cur, M = case([("ground", 0), WALL], [("ground", 0), moved_wall])
    color, cnt = history()
    wall = erode(cur[1][..., 3] == 3, 2)
    assert wall.sum() > 100
    with_table = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam, mesh_motion=table(3, m2=translation(dx=-dx)))
    plain = reproject_ref(color, cnt, *prev, *cur, M, *cam)
    xs = np.broadcast_to(np.arange(W, dtype=np.float64), (H, W))
    # the wall moved one pixel to the right: a wall pixel x shows the texel that was at x - 1.  q is computed in float32 from numbers of
    # magnitude W, so it is within 1e-4 of the integer; the ramp has slope 1 and the count is uniform
    assert (with_table["count"][..., 0][wall] > 0).all()
    assert np.abs(with_table["color"][..., 0][wall] - (xs[wall] - 1)).max() < 1e-3
    assert np.abs(with_table["count"][..., 0][wall] - 16.0).max() < 1e-3
    assert np.abs(with_table["motion"][..., 0][wall] + 1.0).max() < 1e-3 and np.abs(with_table["motion"][..., 1][wall]).max() < 1e-3
    assert with_table["moved"][wall].all()
    # plain reprojection cannot see an in-plane move (same id, normal and plane): it keeps the history UNSHIFTED, i.e. the image slides
    assert (plain["count"][..., 0][wall] > 0).all()
    assert np.abs(plain["color"][..., 0][wall] - xs[wall]).max() < 1e-3
    # the still ground is untouched by the table, bit for bit
    ground = cur[1][..., 3] == 1
    for key in ("color", "count", "motion"):
        assert with_table[key][ground].tobytes() == plain[key][ground].tobytes(), key


def test_move_across_the_plane_test_keeps_the_history_with_the_table_and_loses_it_without():
    dz = 0.5                                                     # > plane_threshold * z = 0.02 * 16.5
    moved_wall = ("wall", WALL[1] + dz, WALL[2], WALL[3], WALL[4])
    cam, prev, cur, M = case([("ground", 0), WALL], [("ground", 0), moved_wall])
    color, cnt = history(1)
    assert dz > 0.02 * float(cur[0][..., 3][cur[1][..., 3] == 3].max())
    # a wall point 4 units off axis moves 4/16 - 4/16.5 of the focal length on screen: under one pixel here, so two pixels inside the
    # wall's outline every tap of the footprint lies on the old wall
    wall = erode(cur[1][..., 3] == 3, 2)
    assert wall.sum() > 100
    with_table = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam, mesh_motion=table(3, m2=translation(dz=-dz)))
    plain = reproject_ref(color, cnt, *prev, *cur, M, *cam)
    assert (with_table["count"][..., 0][wall] > 0).all()
    assert np.abs(with_table["count"][..., 0][wall] - 16.0).max() < 1e-3
    assert (plain["count"][..., 0][cur[1][..., 3] == 3] == 0).all()


def test_moved_sphere_keeps_its_visible_part_and_uncovered_ground_has_no_history():
    step = 0.5
    c = SPHERE[1]
    moved_sphere = ("sphere", (c[0] + step, c[1], c[2]), SPHERE[2], SPHERE[3])
    cam, prev, cur, M = case([("ground", 0), SPHERE, WALL], [("ground", 0), moved_sphere, WALL])
    color, cnt = history(2)
    res = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam, sphere_motion=table(2, m1=translation(dx=-step)))
    sphere = cur[1][..., 3] == 2
    inner = erode(sphere, 1)
    assert inner.sum() > 50 and res["moved"][sphere].all()
    # the sphere is 11 units away and moves 0.5 sideways: the view direction onto it turns by 2.6 degrees, so the newly visible crescent
    # is r * (1 - cos 2.6 deg) = 0.001 units wide, far below a pixel: one pixel inside the outline everything was visible before
    assert (res["count"][..., 0][inner] > 0).mean() >= 0.95
    uncovered = (prev[1][..., 3] == 2) & (cur[1][..., 3] != 2)
    assert uncovered.sum() > 20
    assert (res["count"][..., 0][uncovered] == 0).all() and (res["color"][uncovered] == 0).all()
    # without the table the sphere's history is looked up where the sphere is now: wrong surface points, most of them rejected or smeared
    plain = reproject_ref(color, cnt, *prev, *cur, M, *cam)
    assert (plain["count"][..., 0][inner] > 0).mean() < (res["count"][..., 0][inner] > 0).mean()


def test_identity_tables_and_no_tables_reproduce_plain_reprojection_bit_for_bit():
    cam_a, cam_b = scenes.camera_matrices(W, H), scenes.camera_matrices(W, H, position=(0.35, 1.2, -9.6), yaw_deg=4.0)
    prev, cur = analytic_aovs(W, H, *cam_a), analytic_aovs(W, H, *cam_b)
    rng = np.random.default_rng(4)
    color = (10.0 ** rng.uniform(-3, 2, (H, W, 4))).astype(F)
    cnt = np.zeros((H, W, 4), F)
    cnt[..., 0] = rng.choice([0.0, 1.0, 3.5, 17.0, 64.0, 200.0], (H, W))
    M = scenes.world_to_clip(*cam_a)
    plain = reproject_ref(color, cnt, *prev, *cur, M, *cam_b)
    for kw in (dict(), dict(mesh_motion=table(6), sphere_motion=table(6)), dict(mesh_motion=table(6), moved_max_history=2.0)):
        got = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam_b, **kw)
        for key in ("color", "count", "motion"):
            assert got[key].tobytes() == plain[key].tobytes(), (key, sorted(kw))
        assert not got["moved"].any()


def test_moved_max_history_clamps_moved_pixels_only():
    cam = scenes.camera_matrices(W, H)
    dx = pixel_width_at(cam, WALL[1])
    moved_wall = ("wall", WALL[1], (WALL[2][0] + dx, WALL[2][1] + dx), WALL[3], WALL[4])
    cam, prev, cur, M = case([("ground", 0), SPHERE, WALL], [("ground", 0), SPHERE, moved_wall])
    color, cnt = history(5, count=40.0)
    kw = dict(mesh_motion=table(3, m2=translation(dx=-dx)), sphere_motion=table(2))
    free = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam, max_history=32.0, **kw)
    clamped = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam, max_history=32.0, moved_max_history=4.0, **kw)
    wall = (cur[1][..., 3] == 3) & (free["count"][..., 0] > 0)
    rest = cur[1][..., 3] != 3
    assert wall.sum() > 100
    assert (free["count"][..., 0][wall] == 32.0).all() and (clamped["count"][..., 0][wall] == 4.0).all()
    assert clamped["count"][rest].tobytes() == free["count"][rest].tobytes() and (free["count"][..., 0][rest] == 32.0).any()
    assert clamped["color"].tobytes() == free["color"].tobytes() and clamped["motion"].tobytes() == free["motion"].tobytes()


@pytest.mark.parametrize("bad", ["short_table", "nan_entry", "inf_translation", "zero_matrix"])
def test_out_of_range_ids_and_unusable_entries_give_no_history(bad):
    cam, prev, cur, M = case([("ground", 0), SPHERE, WALL], [("ground", 0), SPHERE, WALL])
    color, cnt = history(6)
    entry = {"nan_entry": np.full(12, np.nan, F), "inf_translation": translation(dx=np.inf), "zero_matrix": np.zeros(12, F)}.get(bad)
    tab = table(2) if bad == "short_table" else table(3, m2=entry)        # the wall is MeshObject 2: a table of two entries has none for it
    res = reproject_objects_ref(color, cnt, *prev, *cur, M, *cam, mesh_motion=tab)
    plain = reproject_ref(color, cnt, *prev, *cur, M, *cam)
    wall = cur[1][..., 3] == 3
    assert wall.sum() > 100 and (plain["count"][..., 0][wall] > 0).all()
    for key in ("color", "count", "motion"):
        assert (res[key][wall] == 0).all(), key
        assert res[key][~wall].tobytes() == plain[key][~wall].tobytes(), key     # spheres (no sphere table), ground and sky: as before


def test_the_quality_move_covers_enough_of_the_image():
    """The GPU quality test evaluates the pixels of the moved objects and requires them to cover 5 % of the image.  Checked here
    without a GPU on analytic stand-ins after the move: the moved sphere itself, and for the moved icosphere (unit radius, level 1) the
    sphere inscribed in it (radius 0.79), so that the count is a lower bound; the other spheres may occlude them."""
    from reproject_motion_ref import QUALITY_CAMERA, QUALITY_MESH, QUALITY_MESH_POSE, QUALITY_MIN_COVERAGE, QUALITY_SIZE, QUALITY_SPHERE, QUALITY_SPHERE_STEP
    w, h = QUALITY_SIZE
    sc = scenes.mixed_test_scene(w, h)
    assert np.allclose(np.asarray(sc.mesh_objects[QUALITY_MESH]["localToWorldMatrix"]).reshape(4, 4)[3, :3], (2.5, 1.0, -1.0))
    objs = [("ground", 0)]
    for i, s in enumerate(sc.spheres):
        c = s["position"].astype(np.float64) + (np.asarray(QUALITY_SPHERE_STEP) if i == QUALITY_SPHERE else 0.0)
        objs.append(("sphere", tuple(c), float(s["radius"]), i))
    objs.append(("sphere", QUALITY_MESH_POSE["translate"], 0.79, 100))
    _, normal, ids = analytic_aovs(w, h, *scenes.camera_matrices(w, h, position=QUALITY_CAMERA), objects=objs)
    o = ids.view(np.int32)[..., 0]
    cover = float((((o == QUALITY_SPHERE) | (o == 100)) & (normal[..., 3] == 2)).mean())
    assert cover >= 1.5 * QUALITY_MIN_COVERAGE, cover
