"""CPU: the motion-blur entry point (include/urt.h urt_motion_blur) — the header compiles as C99, urt_MotionBlurParams has one layout
in gcc, ctypes and the C# binding, the defaults agree from the header's macros to the C# shim, the symbol is exported, a NULL context is
rejected without a device, and the Python wrappers validate their arguments before they call the library."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import motion_blur_ref
from unityraytracer_amd import RayTraceMaster, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
F = np.float32
FIELDS = ("shutter", "max_radius", "flags", "reserved")
DEFAULTS = {"shutter": 0.5, "max_radius": 16.0, "flags": 0}
NAN, INF = float("nan"), float("inf")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "urt.h"\n'
                    'int (*fd)(urt_context*, urt_handle, urt_handle, urt_handle, urt_handle, const urt_MotionBlurParams*) = urt_motion_blur;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(urt_MotionBlurParams, {f})" for f in FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   f'  size_t b[] = {{sizeof(urt_MotionBlurParams), {offs}}};\n'
                   '  for (unsigned k = 0; k < sizeof b / sizeof b[0]; k++) printf("%zu ", b[k]);\n  printf("\\n");\n'
                   '  printf("%a %a %a %d\\n", URT_MOTION_BLUR_DEFAULT_SHUTTER, URT_MOTION_BLUR_DEFAULT_MAX_RADIUS,\n'
                   '         URT_MOTION_BLUR_MAX_RADIUS, URT_MOTION_BLUR_FLAG_VELOCITY);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    b = [int(v) for v in out[0].split()]
    assert b[0] == C.sizeof(_lib.MotionBlurParams) == 16
    assert b[1:] == [getattr(_lib.MotionBlurParams, f).offset for f in FIELDS] == [0, 4, 8, 12]
    v = out[1].split()
    d = _lib.MOTION_BLUR_DEFAULTS
    assert [float.fromhex(x) for x in v[:2]] == [d["shutter"], d["max_radius"]] == [DEFAULTS["shutter"], DEFAULTS["max_radius"]]
    assert float.fromhex(v[2]) == _lib.URT_MOTION_BLUR_MAX_RADIUS == 16.0 == motion_blur_ref.MAX_RADIUS
    assert int(v[3]) == _lib.URT_MOTION_BLUR_FLAG_VELOCITY == motion_blur_ref.FLAG_VELOCITY == 1


def test_declarations_and_defaults_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_motion_blur\(urt_context\* ctx, urt_handle src, urt_handle motion, urt_handle hit, urt_handle dst,\s+"
                     r"const urt_MotionBlurParams\* params\);", text)
    body = re.search(r"typedef struct urt_MotionBlurParams \{(.*?)\} urt_MotionBlurParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(int32_t|uint32_t|float) (\w+);", body, re.M) == \
        [("float", "shutter"), ("float", "max_radius"), ("int32_t", "flags"), ("int32_t", "reserved")]
    assert tuple(n for n, _ in _lib.MotionBlurParams._fields_) == FIELDS
    assert "urt_motion_blur" in _lib.ABI_SYMBOLS
    assert re.search(r"#define URT_MOTION_BLUR_FLAG_VELOCITY 1\b", text) and re.search(r"#define URT_MOTION_BLUR_MAX_RADIUS 16\.0f\b", text)
    # the section sits between the depth of field and the bloom, as the calls are ordered
    k = text.index("/* ---- motion blur")
    assert text.index("/* ---- depth of field") < k < text.index("/* ---- bloom")
    assert "urt_abi_version() == 4" in open(os.path.join(ROOT, "tests", "test_abi.py")).read()            # the version stays what it is
    mh = open(os.path.join(ROOT, "unityraytracer_amd", "csrc", "motion_blur.h")).read()
    assert int(re.search(r"constexpr int kMotionBlurMaxReach = (\d+);", mh).group(1)) == 16
    # C#
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_motion_blur\(IntPtr ctx, ulong src, ulong motion, ulong hit, "
                     r"ulong dst, in MotionBlurParams p\);", cs)
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct MotionBlurParams \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# MotionBlurParams struct is missing"
    assert re.findall(r"public (int|uint|float) (\w+);", m.group(1)) == \
        [("float", "shutter"), ("float", "maxRadius"), ("int", "flags"), ("int", "reserved")]
    d = _lib.MOTION_BLUR_DEFAULTS
    assert f"MotionBlurDefaultShutter = {d['shutter']}f, MotionBlurDefaultMaxRadius = {d['max_radius']}f" in cs
    assert "MotionBlurFlagVelocity = 1" in cs and "MotionBlurMaxRadius = 16.0f" in cs
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert re.search(r"^public static class UrtMotionBlur \{", shim, re.M)
    assert f"float shutter = {d['shutter']}f, float maxRadius = {d['max_radius']}f, bool showVelocity = false" in shim
    assert "UrtNative.urt_motion_blur(ctx, " in shim


def test_reference_and_wrapper_defaults_are_the_library_ones():
    d = _lib.MOTION_BLUR_DEFAULTS
    assert tuple(d) == FIELDS[:3] and d == DEFAULTS
    sig = inspect.signature(motion_blur_ref.motion_blur_ref).parameters
    assert {k: sig[k].default for k in d} == d
    assert list(sig)[:3] == ["src", "motion", "hit"]
    p = unity_api.motion_blur_params()
    assert [getattr(p, k) for k in FIELDS] == [0.5, 16.0, 0, 0]
    sig = inspect.signature(unity_api.Context.motion_blur).parameters
    assert list(sig)[1:] == ["src", "motion", "hit", "dst", "params"] and sig["params"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(RayTraceMaster.EnableMotionBlur).parameters
    assert list(sig)[1:] == ["params"] and sig["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(RayTraceMaster.DisableMotionBlur).parameters) == ["self"]
    sig = inspect.signature(RayTraceMaster.ToneMap).parameters                 # unchanged by the motion blur
    assert list(sig)[1:] == ["destination", "operator", "exposure", "white"]


def test_symbol_is_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_motion_blur")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_motion_blur\b", out)


def test_null_context_is_rejected_and_the_version_stays(built_library):
    lib = _lib.load()
    assert lib.urt_abi_version() == 4
    p = _lib.MotionBlurParams(0.5, 16.0, 0, 0)
    assert lib.urt_motion_blur(None, 1, 2, 3, 4, C.byref(p)) == 1             # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_motion_blur(None, 0, 0, 0, 0, None) == 1


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_motion_blur(self, ctx, src, motion, hit, dst, params):
        p = params._obj
        self.calls.append(("motion_blur", src, motion, hit, dst, tuple(getattr(p, k) for k in FIELDS)))
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
    "unknown_parameter": (TypeError, {"samples": 4}), "reserved_is_no_parameter": (TypeError, {"reserved": 0}),
    "shutter_negative": (ValueError, {"shutter": -0.01}), "shutter_above_1": (ValueError, {"shutter": 1.001}),
    "shutter_nan": (ValueError, {"shutter": NAN}), "shutter_inf": (ValueError, {"shutter": INF}),
    "shutter_str": (TypeError, {"shutter": "0.5"}), "shutter_bool": (TypeError, {"shutter": True}), "shutter_none": (TypeError, {"shutter": None}),
    "radius_small": (ValueError, {"max_radius": 0.25}), "radius_zero": (ValueError, {"max_radius": 0.0}),
    "radius_large": (ValueError, {"max_radius": 16.5}), "radius_nan": (ValueError, {"max_radius": NAN}),
    "radius_inf": (ValueError, {"max_radius": INF}), "radius_str": (TypeError, {"max_radius": "8"}),
    "flags_unknown_bit": (ValueError, {"flags": 2}), "flags_negative": (ValueError, {"flags": -1}), "flags_float": (TypeError, {"flags": 1.0}),
    "flags_bool": (TypeError, {"flags": True}),
}
CALL_BAD = {
    **PARAMS_BAD,
    "src_int": (TypeError, {"src": 7}),
    "motion_none": (TypeError, {"motion": None}),
    "hit_none": (TypeError, {"hit": None}),
    "dst_none": (TypeError, {"dst": None}),
    "dst_other_context": (ValueError, {"dst": "other"}),
    "dst_released": (ValueError, {"dst": "released"}),
    "dst_size": (ValueError, {"dst": "odd"}),
    "motion_size": (ValueError, {"motion": "odd"}),
    "hit_size": (ValueError, {"hit": "odd"}),
    "dst_is_src": (ValueError, {"dst": "src"}),
    "dst_is_motion": (ValueError, {"dst": "motion"}),
    "dst_is_hit": (ValueError, {"dst": "hit"}),
}


@pytest.mark.parametrize("case", sorted(PARAMS_BAD))
def test_motion_blur_params_refuses_each_field_out_of_range(case):
    exc, change = PARAMS_BAD[case]
    with pytest.raises(exc):
        unity_api.motion_blur_params(**change)


def test_motion_blur_params_takes_the_limits():
    for kw in ({"shutter": 0.0}, {"shutter": 1.0}, {"max_radius": 0.5}, {"max_radius": 16.0}, {"flags": _lib.URT_MOTION_BLUR_FLAG_VELOCITY}):
        p = unity_api.motion_blur_params(**kw)
        (k, v), = kw.items()
        assert getattr(p, k) == v and p.reserved == 0


@pytest.mark.parametrize("case", sorted(CALL_BAD))
def test_wrapper_rejects_bad_arguments_before_the_library(stub, case):
    exc, change = CALL_BAD[case]
    kw = {"src": stub_texture(stub, 11, 9, 7), "motion": stub_texture(stub, 12, 9, 7), "hit": stub_texture(stub, 13, 9, 7),
          "dst": stub_texture(stub, 14, 9, 7)}
    textures = {"other": (_other_context(), 99, 9, 7), "released": (stub, 0, 9, 7), "odd": (stub, 98, 2, 2)}
    for k, v in change.items():
        kw[k] = kw[v] if v in ("src", "motion", "hit") else stub_texture(*textures[v]) if isinstance(v, str) and v in textures else v
    with pytest.raises(exc):
        stub.motion_blur(**kw)
    assert stub.lib.calls == []


def test_wrapper_passes_valid_calls(stub):
    src, motion, hit, dst = (stub_texture(stub, 11 + k, 9, 7) for k in range(4))
    stub.motion_blur(src, motion, hit, dst)
    stub.motion_blur(src, motion, hit, dst, shutter=1.0, max_radius=0.5, flags=1)
    stub.motion_blur(src, src, src, dst, shutter=0.0)                         # (the inputs are only read: any may stand in for another)
    assert stub.lib.calls == [("motion_blur", 11, 12, 13, 14, (0.5, 16.0, 0, 0)),
                              ("motion_blur", 11, 12, 13, 14, (1.0, 0.5, 1, 0)),
                              ("motion_blur", 11, 11, 11, 14, (0.0, 16.0, 0, 0))]


def test_master_enable_motion_blur_checks_at_once_and_needs_temporal_accumulation(stub):
    m = object.__new__(RayTraceMaster)
    m.ctx = stub
    m._temporal = {"max_history": 0.0, "normal_threshold": 0.9, "plane_threshold": 0.02}
    assert m._mblur is None and m._mbMotion is None and m._mbStage is None and m._mbAge is None
    for kw, exc in (({"shutter": 2.0}, ValueError), ({"samples": 8}, TypeError), ({"max_radius": 17.0}, ValueError),
                    ({"shutter": "open"}, TypeError), ({"flags": 4}, ValueError)):
        with pytest.raises(exc):
            m.EnableMotionBlur(**kw)
    assert m._mblur is None and m._mbMotion is None and stub.lib.calls == []     # nothing created, nothing called
    m.EnableMotionBlur(shutter=1.0, max_radius=4.0)
    assert m._mblur == {"shutter": 1.0, "max_radius": 4.0} and m._mbMotion is None and m._mbAge is None and stub.lib.calls == []
    m.DisableMotionBlur()
    assert m._mblur is None
    m._temporal = None                                                        # without a reprojection there are no motion vectors
    with pytest.raises(ValueError, match="temporal accumulation"):
        m.EnableMotionBlur()
    assert m._mblur is None
