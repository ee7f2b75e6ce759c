"""CPU: the depth-of-field entry point (include/urt.h urt_depth_of_field) — the header compiles as C99, urt_DofParams has one layout in
gcc, ctypes and the C# binding, the defaults agree from the header's macros to the C# shim, the symbol is exported, a NULL context is
rejected without a device, and the Python wrappers validate their arguments before they call the library."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dof_ref
from unityraytracer_amd import RayTraceMaster, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
F = np.float32
DOF_FIELDS = ("focus_distance", "scale", "max_radius", "flags")
DEFAULTS = {"focus_distance": 10.0, "scale": 8.0, "max_radius": 8.0, "flags": 0}
NAN, INF = float("nan"), float("inf")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "urt.h"\n'
                    'int (*fd)(urt_context*, urt_handle, urt_handle, urt_handle, const urt_DofParams*) = urt_depth_of_field;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(urt_DofParams, {f})" for f in DOF_FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   f'  size_t b[] = {{sizeof(urt_DofParams), {offs}}};\n'
                   '  for (unsigned k = 0; k < sizeof b / sizeof b[0]; k++) printf("%zu ", b[k]);\n  printf("\\n");\n'
                   '  printf("%a %a %a %a %d %d\\n", URT_DOF_DEFAULT_FOCUS_DISTANCE, URT_DOF_DEFAULT_SCALE, URT_DOF_DEFAULT_MAX_RADIUS,\n'
                   '         URT_DOF_MAX_RADIUS, URT_DOF_DEFAULT_FLAGS, URT_DOF_FLAG_COC);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    b = [int(v) for v in out[0].split()]
    assert b[0] == C.sizeof(_lib.DofParams) == 16
    assert b[1:] == [getattr(_lib.DofParams, f).offset for f in DOF_FIELDS] == [0, 4, 8, 12]
    v = out[1].split()
    d = _lib.DOF_DEFAULTS
    assert [float.fromhex(x) for x in v[:3]] == [float(F(d[k])) for k in DOF_FIELDS[:3]] == [float(F(DEFAULTS[k])) for k in DOF_FIELDS[:3]]
    assert float.fromhex(v[3]) == _lib.URT_DOF_MAX_RADIUS == 16.0 == dof_ref.MAX_REACH
    assert [int(x) for x in v[4:]] == [d["flags"], _lib.URT_DOF_FLAG_COC] == [0, 1]
    assert dof_ref.FLAG_COC == 1


def test_declarations_and_defaults_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_depth_of_field\(urt_context\* ctx, urt_handle src, urt_handle hit, urt_handle dst, "
                     r"const urt_DofParams\* params\);", text)
    body = re.search(r"typedef struct urt_DofParams \{(.*?)\} urt_DofParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(int32_t|uint32_t|float) (\w+);", body, re.M) == \
        [("float", n) for n in DOF_FIELDS[:3]] + [("int32_t", "flags")]
    assert tuple(n for n, _ in _lib.DofParams._fields_) == DOF_FIELDS
    assert "urt_depth_of_field" in _lib.ABI_SYMBOLS
    assert re.search(r"#define URT_DOF_FLAG_COC 1\b", text) and re.search(r"#define URT_DOF_MAX_RADIUS 16\.0f\b", text)
    # the section sits between the tone mapping and the bloom, as the calls are ordered
    sections = re.findall(r"^/\* ---- ([a-z\- ]+?) -+ \*/$", text, re.M)
    k = sections.index("depth of field")
    assert sections[k - 1] == "auto-exposure and tone mapping" and sections[k + 1] == "bloom"
    assert "urt_abi_version() == 4" in open(os.path.join(ROOT, "tests", "test_abi.py")).read()            # the version stays what it is
    # the launch constant the header's range of `max_radius` relies on
    dh = open(os.path.join(ROOT, "unityraytracer_amd", "csrc", "dof.h")).read()
    assert int(re.search(r"constexpr int kDofMaxReach = (\d+);", dh).group(1)) == 16
    # C#
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_depth_of_field\(IntPtr ctx, ulong src, ulong hit, ulong dst, "
                     r"in DofParams p\);", cs)
    camel = lambda s: re.sub(r"_(\w)", lambda g: g.group(1).upper(), s)  # noqa: E731
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct DofParams \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# DofParams struct is missing"
    assert re.findall(r"public (int|uint|float) (\w+);", m.group(1)) == [("float", camel(n)) for n in DOF_FIELDS[:3]] + [("int", "flags")]
    d = _lib.DOF_DEFAULTS
    assert (f"DofDefaultFocusDistance = {d['focus_distance']}f, DofDefaultScale = {d['scale']}f, "
            f"DofDefaultMaxRadius = {d['max_radius']}f") in cs
    assert f"DofDefaultFlags = {d['flags']}" in cs and "DofFlagCoc = 1" in cs and "DofMaxRadius = 16.0f" in cs
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert re.search(r"^public static class UrtDepthOfField \{", shim, re.M)
    assert (f"float focusDistance = {d['focus_distance']}f, float scale = {d['scale']}f, float maxRadius = {d['max_radius']}f, "
            f"bool showCoc = false") in shim
    assert "UrtNative.urt_depth_of_field(ctx, " in shim


def test_reference_and_wrapper_defaults_are_the_library_ones():
    d = _lib.DOF_DEFAULTS
    assert tuple(d) == DOF_FIELDS and d == DEFAULTS
    sig = inspect.signature(dof_ref.dof_ref).parameters
    assert {k: sig[k].default for k in DOF_FIELDS} == d
    assert list(sig)[:2] == ["src", "hit"]
    p = unity_api.dof_params()
    assert [getattr(p, k) for k in DOF_FIELDS] == [10.0, 8.0, 8.0, 0]
    sig = inspect.signature(unity_api.Context.depth_of_field).parameters
    assert list(sig)[1:] == ["src", "hit", "dst", "params"] and sig["params"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(RayTraceMaster.EnableDepthOfField).parameters
    assert list(sig)[1:] == ["params"] and sig["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(RayTraceMaster.DisableDepthOfField).parameters) == ["self"]
    sig = inspect.signature(RayTraceMaster.ToneMap).parameters                 # unchanged by the depth of field
    assert list(sig)[1:] == ["destination", "operator", "exposure", "white"]


def test_symbol_is_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_depth_of_field")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_depth_of_field\b", out)


def test_null_context_is_rejected_and_the_version_stays(built_library):
    lib = _lib.load()
    assert lib.urt_abi_version() == 4
    p = _lib.DofParams(10.0, 8.0, 8.0, 0)
    assert lib.urt_depth_of_field(None, 1, 2, 3, C.byref(p)) == 1            # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_depth_of_field(None, 0, 0, 0, None) == 1


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_depth_of_field(self, ctx, src, hit, dst, params):
        p = params._obj
        self.calls.append(("depth_of_field", src, hit, dst, tuple(getattr(p, k) for k in DOF_FIELDS)))
        return 0


@pytest.fixture
def stub():
    ctx = object.__new__(unity_api.Context)
    ctx.lib = _StubLib()
    ctx._h = C.c_void_p(1)
    ctx.device = 0
    return ctx


def stub_texture(ctx, handle, w, h):
    t = object.__new__(unity_api.RenderTexture)
    t.ctx, t.handle, t.width, t.height = ctx, handle, w, h
    return t


def _other_context():
    other = object.__new__(unity_api.Context)
    other.device = 0
    return other


PARAMS_BAD = {
    "unknown_parameter": (TypeError, {"aperture": 4}),
    "focus_zero": (ValueError, {"focus_distance": 0.0}), "focus_negative": (ValueError, {"focus_distance": -1.0}),
    "focus_nan": (ValueError, {"focus_distance": NAN}), "focus_inf": (ValueError, {"focus_distance": INF}),
    "focus_overflows_in_float32": (ValueError, {"focus_distance": 1e39}), "focus_underflows_in_float32": (ValueError, {"focus_distance": 1e-60}),
    "focus_str": (TypeError, {"focus_distance": "10"}), "focus_bool": (TypeError, {"focus_distance": True}),
    "scale_negative": (ValueError, {"scale": -0.5}), "scale_nan": (ValueError, {"scale": NAN}), "scale_inf": (ValueError, {"scale": INF}),
    "scale_overflows_in_float32": (ValueError, {"scale": 1e39}), "scale_none": (TypeError, {"scale": None}),
    "radius_small": (ValueError, {"max_radius": 0.25}), "radius_zero": (ValueError, {"max_radius": 0.0}),
    "radius_large": (ValueError, {"max_radius": 16.5}), "radius_nan": (ValueError, {"max_radius": NAN}),
    "radius_inf": (ValueError, {"max_radius": INF}), "radius_str": (TypeError, {"max_radius": "8"}),
    "flags_unknown_bit": (ValueError, {"flags": 2}), "flags_negative": (ValueError, {"flags": -1}), "flags_float": (TypeError, {"flags": 1.0}),
    "flags_bool": (TypeError, {"flags": True}),
}
CALL_BAD = {
    **PARAMS_BAD,
    "src_int": (TypeError, {"src": 7}),
    "hit_none": (TypeError, {"hit": None}),
    "dst_none": (TypeError, {"dst": None}),
    "dst_other_context": (ValueError, {"dst": "other"}),
    "dst_released": (ValueError, {"dst": "released"}),
    "dst_size": (ValueError, {"dst": "odd"}),
    "hit_size": (ValueError, {"hit": "odd"}),
    "dst_is_src": (ValueError, {"dst": "src"}),
    "dst_is_hit": (ValueError, {"dst": "hit"}),
}


@pytest.mark.parametrize("case", sorted(PARAMS_BAD))
def test_dof_params_refuses_each_field_out_of_range(case):
    exc, change = PARAMS_BAD[case]
    with pytest.raises(exc):
        unity_api.dof_params(**change)


def test_dof_params_takes_the_limits():
    for kw in ({"focus_distance": 1.5e-38}, {"focus_distance": 3e38}, {"scale": 0.0}, {"scale": 3e38}, {"max_radius": 0.5},
               {"max_radius": 16.0}, {"flags": _lib.URT_DOF_FLAG_COC}):
        p = unity_api.dof_params(**kw)
        (k, v), = kw.items()
        assert getattr(p, k) == (float(F(v)) if isinstance(v, float) else v)


@pytest.mark.parametrize("case", sorted(CALL_BAD))
def test_wrapper_rejects_bad_arguments_before_the_library(stub, case):
    exc, change = CALL_BAD[case]
    kw = {"src": stub_texture(stub, 11, 9, 7), "hit": stub_texture(stub, 12, 9, 7), "dst": stub_texture(stub, 13, 9, 7)}
    textures = {"other": (_other_context(), 99, 9, 7), "released": (stub, 0, 9, 7), "odd": (stub, 98, 2, 2)}
    for k, v in change.items():
        kw[k] = kw[v] if v in ("src", "hit") else stub_texture(*textures[v]) if isinstance(v, str) and v in textures else v
    with pytest.raises(exc):
        stub.depth_of_field(**kw)
    assert stub.lib.calls == []


def test_wrapper_passes_valid_calls(stub):
    src, hit, dst = stub_texture(stub, 11, 9, 7), stub_texture(stub, 12, 9, 7), stub_texture(stub, 13, 9, 7)
    stub.depth_of_field(src, hit, dst)
    stub.depth_of_field(src, hit, dst, focus_distance=2.5, scale=0.0, max_radius=16.0, flags=1)
    stub.depth_of_field(src, src, dst, max_radius=0.5)                       # (the library reads only hit.w: any texture may stand in)
    assert stub.lib.calls == [("depth_of_field", 11, 12, 13, (10.0, 8.0, 8.0, 0)),
                              ("depth_of_field", 11, 12, 13, (2.5, 0.0, 16.0, 1)),
                              ("depth_of_field", 11, 11, 13, (10.0, 8.0, 0.5, 0))]


def test_master_enable_depth_of_field_checks_at_once(stub):
    m = object.__new__(RayTraceMaster)
    m.ctx = stub
    assert m._dof is None and m._dofHit is None
    for kw, exc in (({"focus_distance": 0.0}, ValueError), ({"aperture": 1.0}, TypeError), ({"max_radius": 17.0}, ValueError),
                    ({"scale": "wide"}, TypeError), ({"flags": 4}, ValueError)):
        with pytest.raises(exc):
            m.EnableDepthOfField(**kw)
    assert m._dof is None and m._dofHit is None and stub.lib.calls == []     # nothing created, nothing called
    m.EnableDepthOfField(focus_distance=3.0, max_radius=4.0)
    assert m._dof == {"focus_distance": 3.0, "max_radius": 4.0} and m._dofHit is None and stub.lib.calls == []
    m.DisableDepthOfField()
    assert m._dof is None


def test_dof_scale_is_the_thin_lens_circle_of_confusion_at_infinity():
    # Unity's physical camera: f = 50 mm, N = 5.6, a 24 mm sensor; focused at 10 m on 1080 rows:
    # 0.5 * 1080 * 0.0025 / (5.6 * 9.95 * 0.024) = 1.35 / 1.33728 = 1.00951...
    k = unity_api.dof_scale(1080, 10.0)
    assert isinstance(k, np.float32) and k == F(1.35 / 1.33728)
    assert abs(float(k) - 1.0095118) < 1e-6
    assert unity_api.dof_scale(24, 2.0, f_number=1.0, focal_length=1.0, sensor_height=1.0) == F(12.0)     # 0.5 * 24 * 1 / (1 * 1 * 1)
    assert unity_api.dof_scale(2160, 10.0) == F(2.0 * 1.35 / 1.33728)          # linear in the image height
    for s in (0.05, 0.01, 0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            unity_api.dof_scale(1080, s)
    for kw in ({"f_number": 0.0}, {"focal_length": -0.05}, {"sensor_height": 0.0}, {"f_number": NAN}):
        with pytest.raises(ValueError):
            unity_api.dof_scale(1080, 10.0, **kw)
    with pytest.raises(TypeError):
        unity_api.dof_scale(1080.0, 10.0)
    with pytest.raises(ValueError):
        unity_api.dof_scale(0, 10.0)
