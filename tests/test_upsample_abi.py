"""CPU: the guide-driven upsampling entry point (include/urt.h urt_upsample) — the header compiles as C99, the two structs have one layout
in gcc, ctypes and the C# binding, the defaults agree, the symbol is exported, a NULL context is rejected without a device, and the Python
wrappers validate their arguments before they call the library."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from upsample_ref import SKY_FROM_ALBEDO, WIDE_FALLBACK, upsample_ref
from unityraytracer_amd import RayTraceMaster, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
F = np.float32
PARAM_FIELDS = ("normal_threshold", "plane_threshold", "count_scale", "flags")
IMAGE_FIELDS = ("low_color", "low_count", "low_hit", "low_normal", "low_id", "hit", "normal", "id", "albedo", "color", "count")
LOW_FIELDS = IMAGE_FIELDS[:5]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "urt.h"\n'
                    'int (*fn)(urt_context*, const urt_UpsampleImages*, const urt_UpsampleParams*) = urt_upsample;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    offs_p = ", ".join(f"offsetof(urt_UpsampleParams, {f})" for f in PARAM_FIELDS)
    offs_i = ", ".join(f"offsetof(urt_UpsampleImages, {f})" for f in IMAGE_FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   f'  size_t p[] = {{sizeof(urt_UpsampleParams), {offs_p}}};\n'
                   f'  size_t q[] = {{sizeof(urt_UpsampleImages), {offs_i}}};\n'
                   '  for (unsigned k = 0; k < sizeof p / sizeof p[0]; k++) printf("%zu ", p[k]);\n  printf("\\n");\n'
                   '  for (unsigned k = 0; k < sizeof q / sizeof q[0]; k++) printf("%zu ", q[k]);\n  printf("\\n");\n'
                   '  printf("%a %a %a %d %d %d\\n", URT_UPSAMPLE_DEFAULT_NORMAL_THRESHOLD, URT_UPSAMPLE_DEFAULT_PLANE_THRESHOLD,\n'
                   '         URT_UPSAMPLE_DEFAULT_COUNT_SCALE, URT_UPSAMPLE_DEFAULT_FLAGS, URT_UPSAMPLE_WIDE_FALLBACK,\n'
                   '         URT_UPSAMPLE_SKY_FROM_ALBEDO);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    p = [int(v) for v in out[0].split()]
    q = [int(v) for v in out[1].split()]
    assert p[0] == C.sizeof(_lib.UpsampleParams) == 16
    assert p[1:] == [getattr(_lib.UpsampleParams, f).offset for f in PARAM_FIELDS] == [0, 4, 8, 12]
    assert q[0] == C.sizeof(_lib.UpsampleImages) == 88
    assert q[1:] == [getattr(_lib.UpsampleImages, f).offset for f in IMAGE_FIELDS] == list(range(0, 88, 8))
    v = out[2].split()
    d = _lib.UPSAMPLE_DEFAULTS
    assert [float.fromhex(x) for x in v[:3]] == [float(F(d[k])) for k in PARAM_FIELDS[:3]]
    assert [int(x) for x in v[3:]] == [d["flags"], _lib.URT_UPSAMPLE_WIDE_FALLBACK, _lib.URT_UPSAMPLE_SKY_FROM_ALBEDO] == [1, 1, 2]
    assert (WIDE_FALLBACK, SKY_FROM_ALBEDO) == (1, 2)


def test_declarations_and_defaults_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_upsample\(urt_context\* ctx, const urt_UpsampleImages\* images, const urt_UpsampleParams\* params\);", text)
    body = re.search(r"typedef struct urt_UpsampleParams \{(.*?)\} urt_UpsampleParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(int32_t|float) (\w+);", body, re.M) == [("float", "normal_threshold"), ("float", "plane_threshold"),
                                                                      ("float", "count_scale"), ("int32_t", "flags")]
    body = re.search(r"typedef struct urt_UpsampleImages \{(.*?)\} urt_UpsampleImages;", text, re.S).group(1)
    names = [n.strip() for line in re.findall(r"urt_handle ([\w, ]+);", body) for n in line.split(",")]
    assert tuple(names) == IMAGE_FIELDS == tuple(n for n, _ in _lib.UpsampleImages._fields_)
    assert "urt_upsample" in _lib.ABI_SYMBOLS
    macros = {k: float(re.search(rf"#define URT_UPSAMPLE_DEFAULT_{k.upper()} ([0-9.]+)f\b", text).group(1)) for k in PARAM_FIELDS[:3]}
    assert macros == {k: _lib.UPSAMPLE_DEFAULTS[k] for k in PARAM_FIELDS[:3]}
    assert re.search(r"#define URT_UPSAMPLE_DEFAULT_FLAGS URT_UPSAMPLE_WIDE_FALLBACK\b", text)
    assert re.search(r"enum \{ URT_UPSAMPLE_WIDE_FALLBACK = 1, URT_UPSAMPLE_SKY_FROM_ALBEDO = 2 \};", text)
    # the thresholds start at the reprojection's own
    assert _lib.UPSAMPLE_DEFAULTS["normal_threshold"] == _lib.REPROJECT_DEFAULTS["normal_threshold"]
    assert _lib.UPSAMPLE_DEFAULTS["plane_threshold"] == _lib.REPROJECT_DEFAULTS["plane_threshold"]
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_upsample\(IntPtr ctx, in UpsampleImages images, in UpsampleParams p\);", cs)
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct UpsampleParams \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# UpsampleParams struct is missing"
    assert re.findall(r"public (int|float) (\w+);", m.group(1)) == [("float", "normalThreshold"), ("float", "planeThreshold"),
                                                                  ("float", "countScale"), ("int", "flags")]
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct UpsampleImages \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# UpsampleImages struct is missing"
    cs_names = [n.strip() for line in re.findall(r"public ulong ([\w, ]+);", m.group(1)) for n in line.split(",")]
    camel = lambda s: re.sub(r"_(\w)", lambda g: g.group(1).upper(), s)  # noqa: E731
    assert cs_names == [camel(f) for f in IMAGE_FIELDS]
    d = _lib.UPSAMPLE_DEFAULTS
    assert (f"UpsampleDefaultNormalThreshold = {d['normal_threshold']}f, UpsampleDefaultPlaneThreshold = {d['plane_threshold']}f, "
            f"UpsampleDefaultCountScale = {d['count_scale']}f") in cs
    assert "UpsampleWideFallback = 1, UpsampleSkyFromAlbedo = 2" in cs
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert re.search(r"^public static class UrtUpscaler \{", shim, re.M)
    assert (f"float normalThreshold = {d['normal_threshold']}f, float planeThreshold = {d['plane_threshold']}f, "
            f"float countScale = {d['count_scale']}f,") in shim
    assert "bool wideFallback = true, bool skyFromAlbedo = false" in shim and "UrtNative.urt_upsample(ctx, in im, in p)" in shim


def test_reference_and_wrapper_defaults_are_the_library_ones():
    d = _lib.UPSAMPLE_DEFAULTS
    sig = inspect.signature(upsample_ref).parameters
    assert {k: sig[k].default for k in PARAM_FIELDS} == d
    sig = inspect.signature(unity_api.Context.upsample).parameters
    assert list(sig)[1:] == ["low_color", "low_hit", "low_normal", "low_id", "hit", "normal", "id", "color", "count", "low_count", "albedo",
                             "normal_threshold", "plane_threshold", "count_scale", "wide_fallback", "sky_from_albedo"]
    assert {k: sig[k].default for k in PARAM_FIELDS[:3]} == {k: d[k] for k in PARAM_FIELDS[:3]}
    assert sig["wide_fallback"].default is True and sig["sky_from_albedo"].default is False
    assert all(sig[k].default is None for k in ("count", "low_count", "albedo"))
    sig = inspect.signature(RayTraceMaster.Upscale).parameters
    assert list(sig)[1:] == ["width", "height", "destination", "fill_holes", "below", "params"]
    assert sig["destination"].default is None and sig["fill_holes"].default is False and sig["below"].default == 1.0


def test_symbol_is_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_upsample")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_upsample\b", out)


def test_null_context_is_rejected(built_library):
    lib = _lib.load()
    im, p = _lib.UpsampleImages(*range(1, 12)), _lib.UpsampleParams(0.9, 0.02, 1.0, 1)
    assert lib.urt_upsample(None, C.byref(im), C.byref(p)) == 1              # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_upsample(None, None, None) == 1


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_upsample(self, ctx, images, params):
        im, p = images._obj, params._obj
        self.calls.append((tuple(getattr(im, n) for n in IMAGE_FIELDS), (p.normal_threshold, p.plane_threshold, p.count_scale, p.flags)))
        return 0


def stub_context():
    ctx = object.__new__(unity_api.Context)
    ctx.lib = _StubLib()
    ctx._h = C.c_void_p(1)
    ctx.device = 0
    return ctx


def stub_texture(ctx, handle, w, h):
    t = object.__new__(unity_api.RenderTexture)
    t.ctx, t.handle, t.width, t.height = ctx, handle, w, h
    return t


def upsample_kwargs(ctx):
    return {n: stub_texture(ctx, 11 + k, *((4, 3) if n in LOW_FIELDS else (9, 7))) for k, n in enumerate(IMAGE_FIELDS)}


def _apply(ctx, kw, change):
    other = stub_context()
    for k, v in change.items():
        if isinstance(v, str) and v == "other":
            v = stub_texture(other, 99, kw[k].width, kw[k].height)
        elif isinstance(v, str) and v == "released":
            v = stub_texture(ctx, 0, kw[k].width, kw[k].height)
        elif isinstance(v, str) and v == "odd":
            v = stub_texture(ctx, 98, 2, 2)
        elif isinstance(v, str) and v.startswith("same:"):
            v = kw[v[5:]]
        kw[k] = v
    return kw


UPSAMPLE_BAD = {
    "low_color_int": (TypeError, {"low_color": 7}),
    "hit_none": (TypeError, {"hit": None}),
    "color_none": (TypeError, {"color": None}),
    "count_numpy": (TypeError, {"count": np.zeros((7, 9, 4), F)}),
    "albedo_int": (TypeError, {"albedo": 3}),
    "low_count_str": (TypeError, {"low_count": "ones"}),
    "other_context": (ValueError, {"low_id": "other"}),
    "released": (ValueError, {"color": "released"}),
    "low_size": (ValueError, {"low_normal": "odd"}),
    "low_count_size": (ValueError, {"low_count": "odd"}),
    "full_size": (ValueError, {"normal": "odd"}),
    "albedo_size": (ValueError, {"albedo": "odd"}),
    "color_has_the_low_size": (ValueError, {"color": "same:low_color"}),
    "color_is_hit": (ValueError, {"color": "same:hit"}),
    "count_is_albedo": (ValueError, {"count": "same:albedo"}),
    "count_is_color": (ValueError, {"count": "same:color"}),
    "normal_threshold_nan": (ValueError, {"normal_threshold": float("nan")}),
    "plane_threshold_str": (TypeError, {"plane_threshold": "0.1"}),
    "count_scale_zero": (ValueError, {"count_scale": 0.0}),
    "count_scale_negative": (ValueError, {"count_scale": -1.0}),
    "count_scale_inf": (ValueError, {"count_scale": float("inf")}),
    "count_scale_nan": (ValueError, {"count_scale": float("nan")}),
    "count_scale_bool": (TypeError, {"count_scale": True}),
    "wide_fallback_int": (TypeError, {"wide_fallback": 1}),
    "sky_from_albedo_none": (TypeError, {"sky_from_albedo": None}),
}


@pytest.mark.parametrize("case", sorted(UPSAMPLE_BAD))
def test_upsample_wrapper_rejects_bad_arguments_before_the_library(case):
    exc, change = UPSAMPLE_BAD[case]
    ctx = stub_context()
    kw = _apply(ctx, upsample_kwargs(ctx), change)
    with pytest.raises(exc):
        ctx.upsample(**kw)
    assert ctx.lib.calls == []


def test_upsample_wrapper_passes_valid_calls():
    ctx = stub_context()
    ctx.upsample(**upsample_kwargs(ctx))
    kw = upsample_kwargs(ctx)
    kw.update(count=None, low_count=None, albedo=None)
    ctx.upsample(**kw, normal_threshold=-1.0, plane_threshold=1e9, count_scale=0.25, wide_fallback=False, sky_from_albedo=True)
    same = {n: stub_texture(ctx, 40 + k, 5, 5) for k, n in enumerate(IMAGE_FIELDS)}     # equal sizes; an input may serve both grids
    same["hit"], same["normal"], same["id"] = same["low_hit"], same["low_normal"], same["low_id"]
    ctx.upsample(**same)
    d = _lib.UPSAMPLE_DEFAULTS
    defaults = (float(F(d["normal_threshold"])), float(F(d["plane_threshold"])), 1.0, 1)
    assert ctx.lib.calls == [(tuple(range(11, 22)), defaults),
                             ((11, 0, 13, 14, 15, 16, 17, 18, 0, 20, 0), (-1.0, float(F(1e9)), 0.25, 2)),
                             ((40, 41, 42, 43, 44, 42, 43, 44, 48, 49, 50), defaults)]


def test_master_upscale_rejects_bad_arguments_before_creating_anything():
    m = object.__new__(RayTraceMaster)
    m._converged, m._currentSample = None, 0
    with pytest.raises(_lib.UrtError):                                       # before the first frame
        m.Upscale(8, 8)
    ctx = stub_context()
    m.ctx = ctx
    m._converged, m._currentSample = stub_texture(ctx, 5, 4, 3), 1
    for args, kw, exc in (((8.0, 8), {}, TypeError), ((8, 0), {}, ValueError), ((True, 8), {}, TypeError), ((8, 8), {"destination": 3}, TypeError),
                          ((8, 8), {"destination": stub_texture(ctx, 6, 8, 9)}, ValueError), ((8, 8), {"fill_holes": 1}, TypeError),
                          ((8, 8), {"below": float("nan")}, ValueError), ((8, 8), {"count_scale": 2.0}, TypeError),
                          ((8, 8), {"normal_threshold": float("nan")}, ValueError), ((8, 8), {"wide_fallback": "yes"}, TypeError)):
        with pytest.raises(exc):
            m.Upscale(*args, **kw)
    assert ctx.lib.calls == [] and m._upaov is None and m._upcount is None
