"""CPU: the auto-exposure and tone-mapping entry points (include/urt.h urt_auto_exposure / urt_tonemap) — the header compiles as C99, the
three structs have one layout in gcc, ctypes and the C# binding, the defaults agree, the symbols are exported, a NULL context is rejected
without a device, and the Python wrappers validate their arguments before they call the library."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tonemap_ref
from unityraytracer_amd import RayTraceMaster, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
F = np.float32
STATE_FIELDS = ("exposure", "target", "counted", "skipped", "hist")
EXPOSURE_FIELDS = ("key", "min_exposure", "max_exposure", "rate", "low_permille", "high_permille")
TONEMAP_FIELDS = ("exposure", "white", "op", "flags")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "urt.h"\n'
                    'int (*fa)(urt_context*, urt_handle, urt_handle, const urt_ExposureParams*, void*) = urt_auto_exposure;\n'
                    'int (*ft)(urt_context*, urt_handle, urt_handle, const urt_TonemapParams*, const void*) = urt_tonemap;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    offs = {t: ", ".join(f"offsetof(urt_{t}, {f})" for f in fields)
            for t, fields in (("ExposureState", STATE_FIELDS), ("ExposureParams", EXPOSURE_FIELDS), ("TonemapParams", TONEMAP_FIELDS))}
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   f'  size_t s[] = {{sizeof(urt_ExposureState), {offs["ExposureState"]}}};\n'
                   f'  size_t e[] = {{sizeof(urt_ExposureParams), {offs["ExposureParams"]}}};\n'
                   f'  size_t t[] = {{sizeof(urt_TonemapParams), {offs["TonemapParams"]}}};\n'
                   '  for (unsigned k = 0; k < sizeof s / sizeof s[0]; k++) printf("%zu ", s[k]);\n  printf("\\n");\n'
                   '  for (unsigned k = 0; k < sizeof e / sizeof e[0]; k++) printf("%zu ", e[k]);\n  printf("\\n");\n'
                   '  for (unsigned k = 0; k < sizeof t / sizeof t[0]; k++) printf("%zu ", t[k]);\n  printf("\\n");\n'
                   '  printf("%a %a %a %a %d %d\\n", URT_EXPOSURE_DEFAULT_KEY, URT_EXPOSURE_DEFAULT_MIN_EXPOSURE, URT_EXPOSURE_DEFAULT_MAX_EXPOSURE,\n'
                   '         URT_EXPOSURE_DEFAULT_RATE, URT_EXPOSURE_DEFAULT_LOW_PERMILLE, URT_EXPOSURE_DEFAULT_HIGH_PERMILLE);\n'
                   '  printf("%a %a %d %d %d %d %d\\n", URT_TONEMAP_DEFAULT_EXPOSURE, URT_TONEMAP_DEFAULT_WHITE, URT_TONEMAP_DEFAULT_OP,\n'
                   '         URT_TONEMAP_DEFAULT_FLAGS, URT_TONEMAP_LINEAR, URT_TONEMAP_REINHARD, URT_TONEMAP_ACES);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    s, e, t = ([int(v) for v in out[k].split()] for k in range(3))
    assert s[0] == C.sizeof(_lib.ExposureState) == 1040
    assert s[1:] == [getattr(_lib.ExposureState, f).offset for f in STATE_FIELDS] == [0, 4, 8, 12, 16]
    assert e[0] == C.sizeof(_lib.ExposureParams) == 24
    assert e[1:] == [getattr(_lib.ExposureParams, f).offset for f in EXPOSURE_FIELDS] == [0, 4, 8, 12, 16, 20]
    assert t[0] == C.sizeof(_lib.TonemapParams) == 16
    assert t[1:] == [getattr(_lib.TonemapParams, f).offset for f in TONEMAP_FIELDS] == [0, 4, 8, 12]
    v = out[3].split()
    d = _lib.EXPOSURE_DEFAULTS
    assert [float.fromhex(x) for x in v[:4]] == [float(F(d[k])) for k in EXPOSURE_FIELDS[:4]] == [float(F(0.18)), 1.0 / 64.0, 64.0, 1.0]
    assert [int(x) for x in v[4:]] == [d["low_permille"], d["high_permille"]] == [100, 950]
    v = out[4].split()
    d = _lib.TONEMAP_DEFAULTS
    assert [float.fromhex(x) for x in v[:2]] == [d["exposure"], d["white"]] == [1.0, 4.0]
    assert [int(x) for x in v[2:]] == [d["op"], d["flags"], _lib.URT_TONEMAP_LINEAR, _lib.URT_TONEMAP_REINHARD, _lib.URT_TONEMAP_ACES] == [2, 0, 0, 1, 2]
    assert (tonemap_ref.LINEAR, tonemap_ref.REINHARD, tonemap_ref.ACES, tonemap_ref.BINS) == (0, 1, 2, 256)


def test_declarations_and_defaults_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_auto_exposure\(urt_context\* ctx, urt_handle src, urt_handle count, const urt_ExposureParams\* params, "
                     r"void\* d_state\);", text)
    assert re.search(r"URT_API int urt_tonemap\(urt_context\* ctx, urt_handle src, urt_handle dst, const urt_TonemapParams\* params, "
                     r"const void\* d_state\);", text)
    fields = lambda name: re.findall(r"^\s*(int32_t|uint32_t|float) (\w+)(?:\[\d+\])?;",  # noqa: E731
                                     re.search(rf"typedef struct urt_{name} \{{(.*?)\}} urt_{name};", text, re.S).group(1), re.M)
    assert fields("ExposureState") == [("float", "exposure"), ("float", "target"), ("uint32_t", "counted"), ("uint32_t", "skipped"),
                                       ("uint32_t", "hist")]
    assert "uint32_t hist[256];" in text
    assert fields("ExposureParams") == [("float", n) for n in EXPOSURE_FIELDS[:4]] + [("int32_t", n) for n in EXPOSURE_FIELDS[4:]]
    assert fields("TonemapParams") == [("float", "exposure"), ("float", "white"), ("int32_t", "op"), ("int32_t", "flags")]
    for t, names in ((_lib.ExposureState, STATE_FIELDS), (_lib.ExposureParams, EXPOSURE_FIELDS), (_lib.TonemapParams, TONEMAP_FIELDS)):
        assert tuple(n for n, _ in t._fields_) == names
    assert "urt_auto_exposure" in _lib.ABI_SYMBOLS and "urt_tonemap" in _lib.ABI_SYMBOLS
    assert re.search(r"enum \{ URT_TONEMAP_LINEAR = 0, URT_TONEMAP_REINHARD = 1, URT_TONEMAP_ACES = 2 \};", text)
    assert re.search(r"#define URT_TONEMAP_DEFAULT_OP URT_TONEMAP_ACES\b", text)
    assert "urt_abi_version() == 4" in open(os.path.join(ROOT, "tests", "test_abi.py")).read()            # the version stays what it is
    # the launch constant the GPU test relies on
    th = open(os.path.join(ROOT, "unityraytracer_amd", "csrc", "tonemap.h")).read()
    assert int(re.search(r"constexpr int kExposureMaxBlocks = (\d+);", th).group(1)) == unity_api.EXPOSURE_MAX_BLOCKS
    # C#
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_auto_exposure\(IntPtr ctx, ulong src, ulong count, in ExposureParams p, "
                     r"IntPtr dState\);", cs)
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_tonemap\(IntPtr ctx, ulong src, ulong dst, in TonemapParams p, "
                     r"IntPtr dState\);", cs)
    camel = lambda s: re.sub(r"_(\w)", lambda g: g.group(1).upper(), s)  # noqa: E731

    def cs_fields(name):
        m = re.search(rf"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct {name} \{{(.*?)\n    \}}", cs, re.S)
        assert m, f"the C# {name} struct is missing"
        return re.findall(r"public (int|uint|float|uint\[\]) (\w+);", m.group(1))
    assert cs_fields("ExposureState") == [("float", "exposure"), ("float", "target"), ("uint", "counted"), ("uint", "skipped"), ("uint[]", "hist")]
    assert "[MarshalAs(UnmanagedType.ByValArray, SizeConst = 256)]\n        public uint[] hist;" in cs
    assert cs_fields("ExposureParams") == [("float", camel(n)) for n in EXPOSURE_FIELDS[:4]] + [("int", camel(n)) for n in EXPOSURE_FIELDS[4:]]
    assert cs_fields("TonemapParams") == [("float", "exposure"), ("float", "white"), ("int", "op"), ("int", "flags")]
    assert "ExposureStateBytes = 1040" in cs and "TonemapLinear = 0, TonemapReinhard = 1, TonemapAces = 2" in cs
    e, t = _lib.EXPOSURE_DEFAULTS, _lib.TONEMAP_DEFAULTS
    assert (f"ExposureDefaultKey = {e['key']}f, ExposureDefaultMinExposure = {e['min_exposure']}f, ExposureDefaultMaxExposure = "
            f"{e['max_exposure']}f, ExposureDefaultRate = {e['rate']}f") in cs
    assert f"ExposureDefaultLowPermille = {e['low_permille']}, ExposureDefaultHighPermille = {e['high_permille']}" in cs
    assert f"TonemapDefaultExposure = {t['exposure']}f, TonemapDefaultWhite = {t['white']}f" in cs
    assert "TonemapDefaultOp = TonemapAces, TonemapDefaultFlags = 0" in cs
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert re.search(r"^public static class UrtToneMapper \{", shim, re.M)
    assert (f"float key = {e['key']}f, float minExposure = {e['min_exposure']}f, float maxExposure = {e['max_exposure']}f, "
            f"float rate = {e['rate']}f,") in shim
    assert f"int lowPermille = {e['low_permille']}, int highPermille = {e['high_permille']}" in shim
    assert f"int op = UrtNative.TonemapAces, float exposure = {t['exposure']}f, float white = {t['white']}f" in shim
    assert "UrtNative.urt_auto_exposure(ctx, " in shim and "UrtNative.urt_tonemap(ctx, " in shim


def test_reference_and_wrapper_defaults_are_the_library_ones():
    e, t = _lib.EXPOSURE_DEFAULTS, _lib.TONEMAP_DEFAULTS
    assert tuple(e) == EXPOSURE_FIELDS and tuple(t) == TONEMAP_FIELDS
    sig = inspect.signature(tonemap_ref.exposure_resolve_ref).parameters
    assert {k: sig[k].default for k in EXPOSURE_FIELDS} == e
    sig = inspect.signature(tonemap_ref.tonemap_ref).parameters
    assert {k: sig[k].default for k in TONEMAP_FIELDS} == t
    p = unity_api.exposure_params()
    assert [getattr(p, k) for k in EXPOSURE_FIELDS] == [float(F(e[k])) for k in EXPOSURE_FIELDS[:4]] + [100, 950]
    p = unity_api.tonemap_params()
    assert [getattr(p, k) for k in TONEMAP_FIELDS] == [1.0, 4.0, 2, 0]
    assert list(inspect.signature(unity_api.Context.auto_exposure).parameters)[1:] == ["src", "state", "count", "params"]
    assert list(inspect.signature(unity_api.Context.tonemap).parameters)[1:] == ["src", "dst", "state", "params"]
    assert list(inspect.signature(unity_api.Context.exposure_state).parameters)[1:] == ["state"]
    sig = inspect.signature(RayTraceMaster.ToneMap).parameters
    assert list(sig)[1:] == ["destination", "operator", "exposure", "white"]
    assert (sig["destination"].default, sig["operator"].default, sig["exposure"].default, sig["white"].default) == (None, "aces", 1.0, 4.0)
    assert list(inspect.signature(RayTraceMaster.EnableAutoExposure).parameters)[1:] == ["params"]
    assert list(inspect.signature(RayTraceMaster.DisableAutoExposure).parameters) == ["self"]
    assert unity_api.TONEMAP_OPERATORS == {"linear": 0, "reinhard": 1, "aces": 2}


def test_symbols_are_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_auto_exposure") and hasattr(lib, "urt_tonemap")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_auto_exposure\b", out) and re.search(r"\bT urt_tonemap\b", out)


def test_null_context_is_rejected(built_library):
    lib = _lib.load()
    e, t = _lib.ExposureParams(0.18, 1.0 / 64.0, 64.0, 1.0, 100, 950), _lib.TonemapParams(1.0, 4.0, 2, 0)
    assert lib.urt_auto_exposure(None, 1, 0, C.byref(e), C.c_void_p(4096)) == 1     # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_auto_exposure(None, 0, 0, None, None) == 1
    assert lib.urt_tonemap(None, 1, 2, C.byref(t), None) == 1
    assert lib.urt_tonemap(None, 0, 0, None, None) == 1


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_auto_exposure(self, ctx, src, count, params, d_state):
        p = params._obj
        self.calls.append(("auto_exposure", src, count, tuple(getattr(p, k) for k in EXPOSURE_FIELDS), d_state.value))
        return 0

    def urt_tonemap(self, ctx, src, dst, params, d_state):
        p = params._obj
        self.calls.append(("tonemap", src, dst, tuple(getattr(p, k) for k in TONEMAP_FIELDS), d_state.value))
        return 0


class _Device:
    def __init__(self, type="cuda", index=0):
        self.type, self.index = type, index


class _StateTensor:
    """What the wrappers ask of a torch tensor, without a device."""
    __module__ = "torch.stub"

    def __init__(self, ptr=0x7000, nbytes=1040, device=None, contiguous=True):
        self._ptr, self._nbytes, self.device, self._contiguous = ptr, nbytes, device or _Device(), contiguous

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._nbytes // 4

    def element_size(self):
        return 4

    def is_contiguous(self):
        return self._contiguous


@pytest.fixture
def stub(monkeypatch):
    synced = []
    monkeypatch.setattr(unity_api, "_sync_torch_stream", synced.append)
    ctx = object.__new__(unity_api.Context)
    ctx.lib = _StubLib()
    ctx._h = C.c_void_p(1)
    ctx.device = 0
    ctx.synced = synced
    return ctx


def stub_texture(ctx, handle, w, h):
    t = object.__new__(unity_api.RenderTexture)
    t.ctx, t.handle, t.width, t.height = ctx, handle, w, h
    return t


def _other_context():
    other = object.__new__(unity_api.Context)
    other.device = 0
    return other


def _build(ctx, kw, change):
    textures = {"other": (_other_context(), 99, 9, 7), "released": (ctx, 0, 9, 7), "odd": (ctx, 98, 2, 2), "huge": (ctx, 97, 65536, 32768)}
    for k, v in change.items():
        kw[k] = stub_texture(*textures[v]) if isinstance(v, str) and v in textures else v
    return kw


NAN, INF = float("nan"), float("inf")
STATE_BAD = {
    "state_none": (TypeError, {"state": None}),
    "state_numpy": (TypeError, {"state": np.zeros(260, np.int32)}),
    "state_int": (TypeError, {"state": 0x7000}),
    "state_on_the_host": (ValueError, {"state": _StateTensor(device=_Device("cpu", None))}),
    "state_on_another_device": (ValueError, {"state": _StateTensor(device=_Device("cuda", 1))}),
    "state_short": (ValueError, {"state": _StateTensor(nbytes=1036)}),
    "state_strided": (ValueError, {"state": _StateTensor(contiguous=False)}),
    "state_misaligned": (ValueError, {"state": _StateTensor(ptr=0x7008)}),
}
EXPOSURE_BAD = {
    **STATE_BAD,
    "src_int": (TypeError, {"src": 7}),
    "src_none": (TypeError, {"src": None}),
    "src_other_context": (ValueError, {"src": "other"}),
    "src_released": (ValueError, {"src": "released"}),
    "src_huge": (ValueError, {"src": "huge", "count": None}),
    "count_numpy": (TypeError, {"count": np.zeros((7, 9, 4), F)}),
    "count_size": (ValueError, {"count": "odd"}),
    "count_other_context": (ValueError, {"count": "other"}),
    "unknown_parameter": (TypeError, {"gamma": 2.2}),
    "key_nan": (ValueError, {"key": NAN}), "key_zero": (ValueError, {"key": 0.0}), "key_inf": (ValueError, {"key": INF}),
    "key_str": (TypeError, {"key": "0.18"}), "key_bool": (TypeError, {"key": True}),
    "min_negative": (ValueError, {"min_exposure": -1.0}), "max_inf": (ValueError, {"max_exposure": INF}),
    "min_above_max": (ValueError, {"min_exposure": 2.0, "max_exposure": 1.0}),
    "rate_nan": (ValueError, {"rate": NAN}), "rate_zero": (ValueError, {"rate": 0.0}), "rate_negative": (ValueError, {"rate": -1.0}),
    "rate_underflows_in_float32": (ValueError, {"rate": 1e-60}),
    "low_float": (TypeError, {"low_permille": 100.0}), "high_bool": (TypeError, {"high_permille": True}),
    "low_negative": (ValueError, {"low_permille": -1}), "low_equals_high": (ValueError, {"low_permille": 950}),
    "high_above_1000": (ValueError, {"high_permille": 1001}),
}
TONEMAP_BAD = {
    **{k: v for k, v in STATE_BAD.items() if k != "state_none"},
    "src_int": (TypeError, {"src": 7}),
    "dst_none": (TypeError, {"dst": None}),
    "dst_other_context": (ValueError, {"dst": "other"}),
    "dst_released": (ValueError, {"dst": "released"}),
    "dst_size": (ValueError, {"dst": "odd"}),
    "unknown_parameter": (TypeError, {"operator": "aces"}),
    "op_unknown_name": (ValueError, {"op": "filmic"}), "op_unknown_number": (ValueError, {"op": 3}), "op_float": (TypeError, {"op": 2.0}),
    "op_bool": (TypeError, {"op": True}),
    "flags_nonzero": (ValueError, {"flags": 1}), "flags_float": (TypeError, {"flags": 0.0}),
    "exposure_nan": (ValueError, {"exposure": NAN}), "exposure_zero": (ValueError, {"exposure": 0.0}),
    "exposure_inf": (ValueError, {"exposure": INF}), "exposure_overflows_in_float32": (ValueError, {"exposure": 1e39}),
    "exposure_str": (TypeError, {"exposure": "1"}),
    "white_small": (ValueError, {"white": 0.009}), "white_large": (ValueError, {"white": 65505.0}), "white_nan": (ValueError, {"white": NAN}),
    "white_none": (TypeError, {"white": None}),
}


@pytest.mark.parametrize("case", sorted(EXPOSURE_BAD))
def test_auto_exposure_wrapper_rejects_bad_arguments_before_the_library(stub, case):
    exc, change = EXPOSURE_BAD[case]
    kw = _build(stub, {"src": stub_texture(stub, 11, 9, 7), "state": _StateTensor(), "count": stub_texture(stub, 12, 9, 7)}, dict(change))
    with pytest.raises(exc):
        stub.auto_exposure(**kw)
    assert stub.lib.calls == [] and stub.synced == []


@pytest.mark.parametrize("case", sorted(TONEMAP_BAD))
def test_tonemap_wrapper_rejects_bad_arguments_before_the_library(stub, case):
    exc, change = TONEMAP_BAD[case]
    kw = _build(stub, {"src": stub_texture(stub, 11, 9, 7), "dst": stub_texture(stub, 13, 9, 7), "state": _StateTensor()}, dict(change))
    with pytest.raises(exc):
        stub.tonemap(**kw)
    assert stub.lib.calls == [] and stub.synced == []


def test_wrappers_pass_valid_calls(stub):
    src, cnt, dst = stub_texture(stub, 11, 9, 7), stub_texture(stub, 12, 9, 7), stub_texture(stub, 13, 9, 7)
    state = _StateTensor(ptr=0x7010, nbytes=4096)
    stub.auto_exposure(src, state)
    stub.auto_exposure(src, state, cnt, key=0.5, min_exposure=0.5, max_exposure=0.5, rate=INF, low_permille=0, high_permille=1000)
    stub.auto_exposure(src, state, count=None, rate=0.25, low_permille=999, high_permille=1000)
    stub.tonemap(src, dst)
    stub.tonemap(src, src, state, op="reinhard", exposure=2.0, white=0.01)
    stub.tonemap(src, dst, None, op=0, white=65504.0, flags=0)
    e = tuple(float(F(_lib.EXPOSURE_DEFAULTS[k])) for k in EXPOSURE_FIELDS[:4])
    assert stub.lib.calls == [("auto_exposure", 11, 0, e + (100, 950), 0x7010),
                              ("auto_exposure", 11, 12, (0.5, 0.5, 0.5, INF, 0, 1000), 0x7010),
                              ("auto_exposure", 11, 0, e[:3] + (0.25, 999, 1000), 0x7010),
                              ("tonemap", 11, 13, (1.0, 4.0, 2, 0), None),
                              ("tonemap", 11, 11, (2.0, float(F(0.01)), 1, 0), 0x7010),
                              ("tonemap", 11, 13, (1.0, 65504.0, 0, 0), None)]
    assert stub.synced == [state] * 4                                       # torch's stream is waited for whenever a state is passed


def test_master_tonemap_rejects_bad_arguments_before_creating_anything(stub):
    m = object.__new__(RayTraceMaster)
    m._converged = None
    with pytest.raises(_lib.UrtError):                                       # before the first frame
        m.ToneMap()
    m.ctx = stub
    m._converged = stub_texture(stub, 5, 4, 3)
    other = stub_texture(_other_context(), 6, 4, 3)
    for kw, exc in (({"destination": 3}, TypeError), ({"destination": other}, ValueError), ({"destination": stub_texture(stub, 6, 8, 9)}, ValueError),
                    ({"destination": stub_texture(stub, 0, 4, 3)}, ValueError), ({"destination": m._converged}, ValueError),
                    ({"operator": "filmic"}, ValueError), ({"operator": 7}, ValueError), ({"operator": None}, TypeError),
                    ({"exposure": 0.0}, ValueError), ({"exposure": "1"}, TypeError), ({"white": 0.0}, ValueError), ({"white": NAN}, ValueError)):
        with pytest.raises(exc):
            m.ToneMap(**kw)
    for kw, exc in (({"key": 0.0}, ValueError), ({"gamma": 1.0}, TypeError), ({"low_permille": 950}, ValueError), ({"rate": "fast"}, TypeError)):
        with pytest.raises(exc):
            m.EnableAutoExposure(**kw)
    assert stub.lib.calls == [] and m._tonemapped is None and m._exposure is None and m._exposureState is None
    # a valid call with a destination goes straight through; _converged is the source, never the destination
    dest = stub_texture(stub, 6, 4, 3)
    assert m.ToneMap(destination=dest, operator="linear", exposure=0.5, white=2.0) is dest
    assert stub.lib.calls == [("tonemap", 5, 6, (0.5, 2.0, 0, 0), None)]
