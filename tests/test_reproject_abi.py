"""CPU: the temporal reprojection entry points (include/urt.h urt_reproject, urt_blit_add_history) — the header compiles as C99, the two
structs have one layout in gcc, ctypes and the C# binding, the defaults agree, the symbols are exported, a NULL context is rejected
without a device, the Python wrappers validate their arguments before they call the library, and the float32 restatement
(tests/reproject_ref.py) passes its own sanity checks."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from reproject_ref import analytic_aovs, blit_add_history_ref, blit_add_ref, reproject_ref
from unityraytracer_amd import RayTraceMaster, _lib, scenes, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
F = np.float32
PARAM_FIELDS = ("prev_world_to_clip", "max_history", "normal_threshold", "plane_threshold", "flags")
IMAGE_FIELDS = ("prev_color", "prev_count", "prev_hit", "prev_normal", "prev_id", "hit", "normal", "id", "color", "count", "motion")
MACROS = {"max_history": "MAX_HISTORY", "normal_threshold": "NORMAL_THRESHOLD", "plane_threshold": "PLANE_THRESHOLD"}


def header_defaults():
    text = open(URT_H).read()
    return {k: float(re.search(rf"#define URT_REPROJECT_DEFAULT_{m} ([0-9.]+)f\b", text).group(1)) for k, m in MACROS.items()}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "urt.h"\n'
                    'int (*fn)(urt_context*, const urt_ReprojectImages*, const urt_ReprojectParams*) = urt_reproject;\n'
                    'int (*fb)(urt_context*, urt_handle, urt_handle, urt_handle, float) = urt_blit_add_history;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    offs_p = ", ".join(f"offsetof(urt_ReprojectParams, {f})" for f in PARAM_FIELDS)
    offs_i = ", ".join(f"offsetof(urt_ReprojectImages, {f})" for f in IMAGE_FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   f'  size_t p[] = {{sizeof(urt_ReprojectParams), {offs_p}}};\n'
                   f'  size_t q[] = {{sizeof(urt_ReprojectImages), {offs_i}}};\n'
                   '  for (unsigned k = 0; k < sizeof p / sizeof p[0]; k++) printf("%zu ", p[k]);\n  printf("\\n");\n'
                   '  for (unsigned k = 0; k < sizeof q / sizeof q[0]; k++) printf("%zu ", q[k]);\n  printf("\\n");\n'
                   '  printf("%a %a %a\\n", URT_REPROJECT_DEFAULT_MAX_HISTORY, URT_REPROJECT_DEFAULT_NORMAL_THRESHOLD,\n'
                   '         URT_REPROJECT_DEFAULT_PLANE_THRESHOLD);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    p = [int(v) for v in out[0].split()]
    q = [int(v) for v in out[1].split()]
    assert p[0] == C.sizeof(_lib.ReprojectParams) == 80
    assert p[1:] == [getattr(_lib.ReprojectParams, f).offset for f in PARAM_FIELDS] == [0, 64, 68, 72, 76]
    assert q[0] == C.sizeof(_lib.ReprojectImages) == 88
    assert q[1:] == [getattr(_lib.ReprojectImages, f).offset for f in IMAGE_FIELDS] == list(range(0, 88, 8))
    got = dict(zip(MACROS, (float.fromhex(v) for v in out[2].split())))
    assert got == {k: float(F(v)) for k, v in _lib.REPROJECT_DEFAULTS.items()}


def test_declarations_and_defaults_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_reproject\(urt_context\* ctx, const urt_ReprojectImages\* images, const urt_ReprojectParams\* params\);", text)
    assert re.search(r"URT_API int urt_blit_add_history\(urt_context\* ctx, urt_handle src, urt_handle dst, urt_handle count, float max_history\);", text)
    body = re.search(r"typedef struct urt_ReprojectParams \{(.*?)\} urt_ReprojectParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(int32_t|float) (\w+)(\[16\])?;", body, re.M) == [("float", "prev_world_to_clip", "[16]"), ("float", "max_history", ""),
                                                                             ("float", "normal_threshold", ""), ("float", "plane_threshold", ""),
                                                                             ("int32_t", "flags", "")]
    body = re.search(r"typedef struct urt_ReprojectImages \{(.*?)\} urt_ReprojectImages;", text, re.S).group(1)
    names = [n.strip() for line in re.findall(r"urt_handle ([\w, ]+);", body) for n in line.split(",")]
    assert tuple(names) == IMAGE_FIELDS
    assert {"urt_reproject", "urt_blit_add_history"} <= set(_lib.ABI_SYMBOLS)
    assert header_defaults() == _lib.REPROJECT_DEFAULTS
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_reproject\(IntPtr ctx, in ReprojectImages images, in ReprojectParams p\);", cs)
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_blit_add_history\(IntPtr ctx, ulong src, ulong dst, ulong count, "
                     r"float maxHistory\);", cs)
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct ReprojectParams \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# ReprojectParams struct is missing"
    assert re.search(r"\[MarshalAs\(UnmanagedType\.ByValArray, SizeConst = 16\)\]\s*public float\[\] prevWorldToClip;", m.group(1))
    assert re.findall(r"public (int|float) (\w+);", m.group(1)) == [("float", "maxHistory"), ("float", "normalThreshold"),
                                                                  ("float", "planeThreshold"), ("int", "flags")]
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct ReprojectImages \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# ReprojectImages struct is missing"
    cs_names = [n.strip() for line in re.findall(r"public ulong ([\w, ]+);", m.group(1)) for n in line.split(",")]
    camel = lambda s: re.sub(r"_(\w)", lambda g: g.group(1).upper(), s)  # noqa: E731
    assert cs_names == [camel(f) for f in IMAGE_FIELDS]
    d = _lib.REPROJECT_DEFAULTS
    assert (f"ReprojectDefaultMaxHistory = {d['max_history']}f, ReprojectDefaultNormalThreshold = {d['normal_threshold']}f, "
            f"ReprojectDefaultPlaneThreshold = {d['plane_threshold']}f") in cs
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert (f"float maxHistory = {d['max_history']}f, float normalThreshold = {d['normal_threshold']}f, "
            f"float planeThreshold = {d['plane_threshold']}f") in shim


def test_reference_and_wrapper_defaults_are_the_header_ones():
    import inspect
    sig = inspect.signature(reproject_ref).parameters
    assert {k: sig[k].default for k in MACROS} == header_defaults()
    sig = inspect.signature(unity_api.Context.reproject).parameters
    assert {k: sig[k].default for k in MACROS} == header_defaults()


def test_symbols_are_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_reproject") and hasattr(lib, "urt_blit_add_history")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_reproject\b", out) and re.search(r"\bT urt_blit_add_history\b", out)


def test_null_context_is_rejected(built_library):
    lib = _lib.load()
    im, p = _lib.ReprojectImages(*range(1, 12)), _lib.ReprojectParams()
    assert lib.urt_reproject(None, C.byref(im), C.byref(p)) == 1          # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_reproject(None, None, None) == 1
    assert lib.urt_blit_add_history(None, 1, 2, 3, 0.0) == 1


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_reproject(self, *a):
        self.calls.append(("reproject",))
        return 0

    def urt_blit_add_history(self, *a):
        self.calls.append(("blit_add_history",) + a[1:])
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


def reproject_kwargs(ctx):
    kw = {n: stub_texture(ctx, 11 + k) for k, n in enumerate(IMAGE_FIELDS)}
    kw["prev_world_to_clip"] = np.eye(4, dtype=F).reshape(16)
    return kw


def _apply(ctx, kw, change):
    other = stub_context()
    for k, v in change.items():
        if isinstance(v, str) and v == "other":
            v = stub_texture(other, 99)
        elif isinstance(v, str) and v == "released":
            v = stub_texture(ctx, 0)
        elif isinstance(v, str) and v == "small":
            v = stub_texture(ctx, 98, 2, 2)
        elif isinstance(v, str) and v.startswith("same:"):
            v = kw[v[5:]]
        kw[k] = v
    return kw


REPROJECT_BAD = {
    "prev_color_int": (TypeError, {"prev_color": 7}),
    "hit_none": (TypeError, {"hit": None}),
    "count_numpy": (TypeError, {"count": np.zeros((3, 4, 4), F)}),
    "motion_int": (TypeError, {"motion": 3}),
    "other_context": (ValueError, {"prev_id": "other"}),
    "released": (ValueError, {"color": "released"}),
    "size": (ValueError, {"normal": "small"}),
    "motion_size": (ValueError, {"motion": "small"}),
    "color_is_input": (ValueError, {"color": "same:prev_color"}),
    "count_is_hit": (ValueError, {"count": "same:hit"}),
    "motion_is_color": (ValueError, {"motion": "same:color"}),
    "count_is_color": (ValueError, {"count": "same:color"}),
    "matrix_15": (ValueError, {"prev_world_to_clip": np.zeros(15, F)}),
    "matrix_str": (TypeError, {"prev_world_to_clip": "eye"}),
    "max_history_half": (ValueError, {"max_history": 0.5}),
    "max_history_negative": (ValueError, {"max_history": -1.0}),
    "max_history_nan": (ValueError, {"max_history": float("nan")}),
    "max_history_bool": (TypeError, {"max_history": True}),
    "normal_threshold_nan": (ValueError, {"normal_threshold": float("nan")}),
    "plane_threshold_str": (TypeError, {"plane_threshold": "0.1"}),
}


@pytest.mark.parametrize("case", sorted(REPROJECT_BAD))
def test_reproject_wrapper_rejects_bad_arguments_before_the_library(case):
    exc, change = REPROJECT_BAD[case]
    ctx = stub_context()
    kw = _apply(ctx, reproject_kwargs(ctx), change)
    with pytest.raises(exc):
        ctx.reproject(**kw)
    assert ctx.lib.calls == []


def test_reproject_wrapper_passes_valid_calls():
    ctx = stub_context()
    ctx.reproject(**reproject_kwargs(ctx))
    kw = reproject_kwargs(ctx)
    kw["motion"] = None
    ctx.reproject(**kw, max_history=0, normal_threshold=-1.0, plane_threshold=1e9)
    ctx.reproject(**reproject_kwargs(ctx), max_history=1.0)
    assert ctx.lib.calls == [("reproject",)] * 3


BLEND_BAD = {
    "src_int": (TypeError, {"src": 5}),
    "count_none": (TypeError, {"count": None}),
    "other_context": (ValueError, {"dst": "other"}),
    "released": (ValueError, {"count": "released"}),
    "size": (ValueError, {"count": "small"}),
    "src_is_dst": (ValueError, {"dst": "same:src"}),
    "count_is_src": (ValueError, {"count": "same:src"}),
    "count_is_dst": (ValueError, {"count": "same:dst"}),
    "max_history_half": (ValueError, {"max_history": 0.25}),
    "max_history_nan": (ValueError, {"max_history": float("nan")}),
    "max_history_negative": (ValueError, {"max_history": -2}),
    "max_history_str": (TypeError, {"max_history": "8"}),
}


@pytest.mark.parametrize("case", sorted(BLEND_BAD))
def test_blend_wrapper_rejects_bad_arguments_before_the_library(case):
    exc, change = BLEND_BAD[case]
    ctx = stub_context()
    kw = {"src": stub_texture(ctx, 1), "dst": stub_texture(ctx, 2), "count": stub_texture(ctx, 3)}
    kw = _apply(ctx, kw, change)
    with pytest.raises(exc):
        ctx.blit_add_history(**kw)
    assert ctx.lib.calls == []
    ctx.blit_add_history(stub_texture(ctx, 1), stub_texture(ctx, 2), stub_texture(ctx, 3), 8)
    assert ctx.lib.calls == [("blit_add_history", 1, 2, 3, 8.0)]


def test_master_rejects_bad_temporal_settings_before_creating_anything():
    m = object.__new__(RayTraceMaster)
    m._temporal = None
    for bad, exc in (({"max_history": 0.5}, ValueError), ({"normal_threshold": float("nan")}, ValueError), ({"plane_threshold": "x"}, TypeError)):
        with pytest.raises(exc):
            m.EnableTemporalAccumulation(**bad)
        assert m._temporal is None


def test_world_to_clip_is_projection_times_world_to_camera():
    c2w, invp = scenes.camera_matrices(64, 40, position=(1.0, 2.0, -7.0), yaw_deg=20.0, pitch_deg=5.0)
    M = scenes.world_to_clip(c2w, invp)
    assert M.dtype == F and M.shape == (16,)
    p = np.array([0.3, 1.1, 2.0, 1.0])
    clip = M.astype(np.float64).reshape(4, 4).T @ p
    cam = np.linalg.inv(c2w.astype(np.float64).reshape(4, 4).T) @ p
    assert clip[3] == pytest.approx(-cam[2], rel=1e-5)                  # GL-style: w = -z of the camera space (Unity looks down -z)
    back = invp.astype(np.float64).reshape(4, 4).T @ clip
    assert np.allclose(back[:3] / back[3], cam[:3] / cam[3], rtol=1e-4, atol=1e-5)


# ---- the reference's own sanity checks -----------------------------------------------------------------------------------------------
W, H = 64, 40


def camera(**kw):
    return scenes.camera_matrices(W, H, **kw)


def history(seed, n=10.0):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0, 1, (H, W, 4)).astype(F)
    count = np.zeros((H, W, 4), F)
    count[..., 0] = n
    return color, count


def run_ref(prev_cam, cur_cam, color, count, prev_aov=None, objects=None, **params):
    prev = analytic_aovs(W, H, *prev_cam, objects=objects) if prev_aov is None else prev_aov
    cur = analytic_aovs(W, H, *cur_cam, objects=objects)
    return reproject_ref(color, count, *prev, *cur, scenes.world_to_clip(*prev_cam), *cur_cam, **params), prev, cur


def test_reference_same_camera_keeps_the_history():
    cam = camera()
    color, count = history(1)
    r, prev, _ = run_ref(cam, cam, color, count)
    assert r["window"].all()
    assert np.abs(r["motion"][..., :2]).max() < 1e-3
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    assert np.allclose(r["color"][inner], color[inner], atol=2e-3)
    assert np.allclose(r["count"][inner][:, 0], 10.0, rtol=1e-5)
    assert (r["count"][..., 1:] == 0).all()


def test_reference_one_pixel_shift_of_a_fronto_parallel_plane():
    objects = [("wall", 10.0, (-100.0, 100.0), (-100.0, 100.0), 7)]      # fills the view at distance 20 from the camera
    cam = camera()
    f = 1.0 / math.tan(math.radians(81.0) * 0.5)
    dist = 10.0 - (-10.0)
    dx = (2.0 / W) * dist * (W / H) / f                                  # one pixel at that distance
    moved = camera(position=(dx, 1.0, -10.0))
    color, count = history(2)
    prev = analytic_aovs(W, H, *cam, objects=objects)
    cur = analytic_aovs(W, H, *moved, objects=objects)
    r = reproject_ref(color, count, *prev, *cur, scenes.world_to_clip(*cam), *moved)
    assert np.allclose(r["motion"][:, :-1, 0], 1.0, atol=1e-3) and np.allclose(r["motion"][:, :-1, 1], 0.0, atol=1e-3)
    assert not r["window"][:, -1].any()                                   # the last column comes from beyond the previous view
    assert np.allclose(r["color"][:, :-2], color[:, 1:-1], atol=2e-3)    # history[x] = prev[x + 1]
    assert np.allclose(r["count"][:, :-2, 0], 10.0, rtol=1e-5)


def test_reference_changed_object_id_has_no_history():
    cam = camera()
    color, count = history(3)
    hit, normal, ids = analytic_aovs(W, H, *cam)
    other = ids.copy()
    other.view(np.int32)[..., 0] += 1000
    r, _, _ = run_ref(cam, cam, color, count, prev_aov=(hit, normal, other))
    surf = normal[..., 3] != 0
    assert surf.any()
    assert (r["count"][surf] == 0).all() and (r["color"][surf] == 0).all()
    assert (r["count"][~surf][:, 0] > 0).all()                            # the sky keeps its history


def test_reference_points_behind_the_previous_camera_have_no_history():
    cam = camera()
    ahead = camera(position=(0.0, 1.0, 8.0))                             # past every object but the far ground, looking the same way
    color, count = history(4)
    r, _, cur = run_ref(ahead, cam, color, count)
    surf = cur[1][..., 3] != 0
    behind_prev = surf & (cur[0][..., 2] < 7.99)                         # behind the previous camera: cw < 0
    assert behind_prev.sum() > 0.5 * surf.sum()
    assert not r["window"][behind_prev].any()
    assert (r["count"][behind_prev] == 0).all() and (r["color"][behind_prev] == 0).all() and (r["motion"][behind_prev] == 0).all()


def test_reference_sky_survives_a_pure_translation():
    cam = camera()
    moved = camera(position=(0.7, 1.4, -9.0))
    color, count = history(5)
    r, _, cur = run_ref(cam, moved, color, count, objects=[("ground", 0)])   # nothing above the horizon: no sky is disoccluded
    sky = cur[1][..., 3] == 0
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    s = sky & inner
    assert s.sum() > 100
    assert np.abs(r["motion"][s][:, :2]).max() < 1e-3
    assert np.allclose(r["count"][s][:, 0], 10.0, rtol=1e-5)


def test_reference_clamps_to_max_history():
    cam = camera()
    color, count = history(6, n=100.0)
    capped, _, _ = run_ref(cam, cam, color, count, max_history=64.0)
    free, _, _ = run_ref(cam, cam, color, count, max_history=0.0)
    h = capped["count"][..., 0] > 0
    assert h.mean() > 0.9
    assert (capped["count"][h][:, 0] == 64.0).all()
    assert np.allclose(free["count"][h][:, 0], 100.0, rtol=1e-5)


def test_reference_uniform_count_blend_is_the_addition_shader():
    rng = np.random.default_rng(7)
    src = rng.uniform(0, 2, (H, W, 4)).astype(F)
    dst = rng.uniform(0, 2, (H, W, 4)).astype(F)
    for n in (0.0, 1.0, 2.0, 7.0, 63.0, 1000.0):
        count = np.zeros((H, W, 4), F)
        count[..., 0] = n
        got, cnt = blit_add_history_ref(src, dst, count, 0.0)
        assert got.view(np.uint32).tobytes() == blit_add_ref(src, dst, n).view(np.uint32).tobytes(), n
        assert (cnt[..., 0] == F(n) + F(1)).all() and (cnt[..., 1:] == 0).all()
    count = np.zeros((H, W, 4), F)
    count[..., 0] = [np.nan, -1.0, np.inf, 200.0][0]
    got, cnt = blit_add_history_ref(src, dst, count, 8.0)
    assert got.tobytes() == blit_add_ref(src, dst, 0.0).tobytes() and (cnt[..., 0] == 1).all()
    count[..., 0] = 200.0
    got, cnt = blit_add_history_ref(src, dst, count, 8.0)
    assert got.tobytes() == blit_add_ref(src, dst, 7.0).tobytes() and (cnt[..., 0] == 8).all()
