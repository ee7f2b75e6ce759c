"""CPU: the bloom entry point (include/urt.h urt_bloom) — the header compiles as C99, urt_BloomParams has one layout in gcc, ctypes and the
C# binding, the defaults agree from the header's macros to the C# shim, the symbol is exported, a NULL context is rejected without a
device, and the Python wrappers validate their arguments before they call the library."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bloom_ref
from unityraytracer_amd import RayTraceMaster, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
F = np.float32
BLOOM_FIELDS = ("threshold", "soft_knee", "clamp", "scatter", "intensity", "levels", "flags")
DEFAULTS = {"threshold": 1.0, "soft_knee": 0.5, "clamp": 65504.0, "scatter": 0.7, "intensity": 0.2, "levels": 6, "flags": 0}
NAN, INF = float("nan"), float("inf")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"
    decl.write_text('#include "urt.h"\n'
                    'int (*fb)(urt_context*, urt_handle, urt_handle, const urt_BloomParams*, const void*) = urt_bloom;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    offs = ", ".join(f"offsetof(urt_BloomParams, {f})" for f in BLOOM_FIELDS)
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   f'  size_t b[] = {{sizeof(urt_BloomParams), {offs}}};\n'
                   '  for (unsigned k = 0; k < sizeof b / sizeof b[0]; k++) printf("%zu ", b[k]);\n  printf("\\n");\n'
                   '  printf("%a %a %a %a %a %d %d %d\\n", URT_BLOOM_DEFAULT_THRESHOLD, URT_BLOOM_DEFAULT_SOFT_KNEE, URT_BLOOM_DEFAULT_CLAMP,\n'
                   '         URT_BLOOM_DEFAULT_SCATTER, URT_BLOOM_DEFAULT_INTENSITY, URT_BLOOM_DEFAULT_LEVELS, URT_BLOOM_DEFAULT_FLAGS,\n'
                   '         URT_BLOOM_FLAG_ONLY);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    b = [int(v) for v in out[0].split()]
    assert b[0] == C.sizeof(_lib.BloomParams) == 28
    assert b[1:] == [getattr(_lib.BloomParams, f).offset for f in BLOOM_FIELDS] == [0, 4, 8, 12, 16, 20, 24]
    v = out[1].split()
    d = _lib.BLOOM_DEFAULTS
    assert [float.fromhex(x) for x in v[:5]] == [float(F(d[k])) for k in BLOOM_FIELDS[:5]] == [float(F(DEFAULTS[k])) for k in BLOOM_FIELDS[:5]]
    assert [int(x) for x in v[5:]] == [d["levels"], d["flags"], _lib.URT_BLOOM_FLAG_ONLY] == [6, 0, 1]
    assert bloom_ref.FLAG_ONLY == 1


def test_declarations_and_defaults_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_bloom\(urt_context\* ctx, urt_handle src, urt_handle dst, const urt_BloomParams\* params, "
                     r"const void\* d_state\);", text)
    body = re.search(r"typedef struct urt_BloomParams \{(.*?)\} urt_BloomParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(int32_t|uint32_t|float) (\w+);", body, re.M) == \
        [("float", n) for n in BLOOM_FIELDS[:5]] + [("int32_t", n) for n in BLOOM_FIELDS[5:]]
    assert tuple(n for n, _ in _lib.BloomParams._fields_) == BLOOM_FIELDS
    assert "urt_bloom" in _lib.ABI_SYMBOLS
    assert re.search(r"#define URT_BLOOM_FLAG_ONLY 1\b", text)
    assert "urt_abi_version() == 4" in open(os.path.join(ROOT, "tests", "test_abi.py")).read()            # the version stays what it is
    # the launch constant the header's range of `levels` relies on
    bh = open(os.path.join(ROOT, "unityraytracer_amd", "csrc", "bloom.h")).read()
    assert int(re.search(r"constexpr int kBloomMaxLevels = (\d+);", bh).group(1)) == 16
    # C#
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_bloom\(IntPtr ctx, ulong src, ulong dst, in BloomParams p, "
                     r"IntPtr dState\);", cs)
    camel = lambda s: re.sub(r"_(\w)", lambda g: g.group(1).upper(), s)  # noqa: E731
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct BloomParams \{(.*?)\n    \}", cs, re.S)
    assert m, "the C# BloomParams struct is missing"
    assert re.findall(r"public (int|uint|float) (\w+);", m.group(1)) == \
        [("float", camel(n)) for n in BLOOM_FIELDS[:5]] + [("int", camel(n)) for n in BLOOM_FIELDS[5:]]
    d = _lib.BLOOM_DEFAULTS
    assert (f"BloomDefaultThreshold = {d['threshold']}f, BloomDefaultSoftKnee = {d['soft_knee']}f, BloomDefaultClamp = {d['clamp']}f, "
            f"BloomDefaultScatter = {d['scatter']}f, BloomDefaultIntensity = {d['intensity']}f") in cs
    assert f"BloomDefaultLevels = {d['levels']}, BloomDefaultFlags = {d['flags']}" in cs and "BloomFlagOnly = 1" in cs
    shim = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    assert re.search(r"^public static class UrtBloom \{", shim, re.M)
    assert (f"float threshold = {d['threshold']}f, float softKnee = {d['soft_knee']}f, float clamp = {d['clamp']}f, "
            f"float scatter = {d['scatter']}f,") in shim
    assert f"float intensity = {d['intensity']}f, int levels = {d['levels']}, bool bloomOnly = false" in shim
    assert "UrtNative.urt_bloom(ctx, " in shim


def test_reference_and_wrapper_defaults_are_the_library_ones():
    d = _lib.BLOOM_DEFAULTS
    assert tuple(d) == BLOOM_FIELDS and d == DEFAULTS
    sig = inspect.signature(bloom_ref.bloom_ref).parameters
    assert {k: sig[k].default for k in BLOOM_FIELDS} == d
    assert list(sig)[:2] == ["src", "exposure"] and sig["exposure"].default is None
    p = unity_api.bloom_params()
    assert [getattr(p, k) for k in BLOOM_FIELDS] == [float(F(d[k])) for k in BLOOM_FIELDS[:5]] + [6, 0]
    sig = inspect.signature(unity_api.Context.bloom).parameters
    assert list(sig)[1:] == ["src", "dst", "state", "params"] and sig["state"].default is None
    assert sig["params"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(RayTraceMaster.EnableBloom).parameters
    assert list(sig)[1:] == ["params"] and sig["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(RayTraceMaster.DisableBloom).parameters) == ["self"]
    sig = inspect.signature(RayTraceMaster.ToneMap).parameters                 # unchanged by the bloom
    assert list(sig)[1:] == ["destination", "operator", "exposure", "white"]


def test_symbol_is_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_bloom")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_bloom\b", out)


def test_null_context_is_rejected_and_the_version_stays(built_library):
    lib = _lib.load()
    assert lib.urt_abi_version() == 4
    p = _lib.BloomParams(1.0, 0.5, 65504.0, 0.7, 0.2, 6, 0)
    assert lib.urt_bloom(None, 1, 2, C.byref(p), None) == 1                  # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_bloom(None, 0, 0, None, None) == 1


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def urt_auto_exposure(self, ctx, src, count, params, d_state):
        self.calls.append(("auto_exposure", src, count, d_state.value))
        return 0

    def urt_bloom(self, ctx, src, dst, params, d_state):
        p = params._obj
        self.calls.append(("bloom", src, dst, tuple(getattr(p, k) for k in BLOOM_FIELDS), d_state.value))
        return 0

    def urt_tonemap(self, ctx, src, dst, params, d_state):
        p = params._obj
        self.calls.append(("tonemap", src, dst, (p.exposure, p.white, p.op, p.flags), d_state.value))
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


PARAMS_BAD = {
    "unknown_parameter": (TypeError, {"radius": 4}),
    "threshold_negative": (ValueError, {"threshold": -0.5}), "threshold_large": (ValueError, {"threshold": 65505.0}),
    "threshold_nan": (ValueError, {"threshold": NAN}), "threshold_inf": (ValueError, {"threshold": INF}),
    "threshold_str": (TypeError, {"threshold": "1"}), "threshold_bool": (TypeError, {"threshold": True}),
    "knee_negative": (ValueError, {"soft_knee": -0.1}), "knee_above_1": (ValueError, {"soft_knee": 1.5}), "knee_nan": (ValueError, {"soft_knee": NAN}),
    "clamp_zero": (ValueError, {"clamp": 0.0}), "clamp_negative": (ValueError, {"clamp": -1.0}), "clamp_large": (ValueError, {"clamp": 70000.0}),
    "clamp_nan": (ValueError, {"clamp": NAN}), "clamp_underflows_in_float32": (ValueError, {"clamp": 1e-60}),
    "scatter_negative": (ValueError, {"scatter": -0.1}), "scatter_above_1": (ValueError, {"scatter": 1.0001}), "scatter_nan": (ValueError, {"scatter": NAN}),
    "intensity_negative": (ValueError, {"intensity": -1.0}), "intensity_nan": (ValueError, {"intensity": NAN}), "intensity_inf": (ValueError, {"intensity": INF}),
    "intensity_overflows_in_float32": (ValueError, {"intensity": 1e39}), "intensity_none": (TypeError, {"intensity": None}),
    "levels_zero": (ValueError, {"levels": 0}), "levels_17": (ValueError, {"levels": 17}), "levels_negative": (ValueError, {"levels": -1}),
    "levels_float": (TypeError, {"levels": 6.0}), "levels_bool": (TypeError, {"levels": True}),
    "flags_unknown_bit": (ValueError, {"flags": 2}), "flags_negative": (ValueError, {"flags": -1}), "flags_float": (TypeError, {"flags": 1.0}),
}
CALL_BAD = {
    **PARAMS_BAD,
    "state_numpy": (TypeError, {"state": np.zeros(260, np.int32)}),
    "state_int": (TypeError, {"state": 0x7000}),
    "state_on_the_host": (ValueError, {"state": _StateTensor(device=_Device("cpu", None))}),
    "state_on_another_device": (ValueError, {"state": _StateTensor(device=_Device("cuda", 1))}),
    "state_short": (ValueError, {"state": _StateTensor(nbytes=1036)}),
    "state_strided": (ValueError, {"state": _StateTensor(contiguous=False)}),
    "state_misaligned": (ValueError, {"state": _StateTensor(ptr=0x7008)}),
    "src_int": (TypeError, {"src": 7}),
    "dst_none": (TypeError, {"dst": None}),
    "dst_other_context": (ValueError, {"dst": "other"}),
    "dst_released": (ValueError, {"dst": "released"}),
    "dst_size": (ValueError, {"dst": "odd"}),
}


@pytest.mark.parametrize("case", sorted(PARAMS_BAD))
def test_bloom_params_refuses_each_field_out_of_range(case):
    exc, change = PARAMS_BAD[case]
    with pytest.raises(exc):
        unity_api.bloom_params(**change)


def test_bloom_params_takes_the_limits():
    for kw in ({"threshold": 0.0}, {"threshold": 65504.0}, {"soft_knee": 0.0}, {"soft_knee": 1.0}, {"clamp": 1e-30}, {"clamp": 65504.0},
               {"scatter": 0.0}, {"scatter": 1.0}, {"intensity": 0.0}, {"intensity": 3e38}, {"levels": 1}, {"levels": 16},
               {"flags": _lib.URT_BLOOM_FLAG_ONLY}):
        p = unity_api.bloom_params(**kw)
        (k, v), = kw.items()
        assert getattr(p, k) == (float(F(v)) if isinstance(v, float) else v)


@pytest.mark.parametrize("case", sorted(CALL_BAD))
def test_bloom_wrapper_rejects_bad_arguments_before_the_library(stub, case):
    exc, change = CALL_BAD[case]
    textures = {"other": (_other_context(), 99, 9, 7), "released": (stub, 0, 9, 7), "odd": (stub, 98, 2, 2)}
    kw = {"src": stub_texture(stub, 11, 9, 7), "dst": stub_texture(stub, 13, 9, 7), "state": _StateTensor()}
    for k, v in change.items():
        kw[k] = stub_texture(*textures[v]) if isinstance(v, str) and v in textures else v
    with pytest.raises(exc):
        stub.bloom(**kw)
    assert stub.lib.calls == [] and stub.synced == []


def test_wrapper_passes_valid_calls(stub):
    src, dst = stub_texture(stub, 11, 9, 7), stub_texture(stub, 13, 9, 7)
    state = _StateTensor(ptr=0x7010, nbytes=4096)
    stub.bloom(src, dst)
    stub.bloom(src, src, state, threshold=0.0, soft_knee=1.0, clamp=4.0, scatter=0.0, intensity=2.0, levels=16, flags=1)
    stub.bloom(src, dst, None, levels=1)
    d = tuple(float(F(DEFAULTS[k])) for k in BLOOM_FIELDS[:5])
    assert stub.lib.calls == [("bloom", 11, 13, d + (6, 0), None),
                              ("bloom", 11, 11, (0.0, 1.0, 4.0, 0.0, 2.0, 16, 1), 0x7010),
                              ("bloom", 11, 13, d + (1, 0), None)]
    assert stub.synced == [state]                                           # torch's stream is waited for whenever a state is passed


def test_master_enable_bloom_checks_at_once_and_tonemap_orders_the_calls(stub):
    m = object.__new__(RayTraceMaster)
    m.ctx = stub
    m._converged = stub_texture(stub, 5, 4, 3)
    assert m._bloom is None
    for kw, exc in (({"threshold": -1.0}, ValueError), ({"radius": 1.0}, TypeError), ({"levels": 0}, ValueError), ({"scatter": "wide"}, TypeError)):
        with pytest.raises(exc):
            m.EnableBloom(**kw)
    assert m._bloom is None and stub.lib.calls == [] and m._tonemapped is None     # nothing created, nothing called
    dest = stub_texture(stub, 6, 4, 3)
    tm = (0.5, 2.0, 0, 0)
    m.ToneMap(destination=dest, operator="linear", exposure=0.5, white=2.0)         # bloom not enabled: today's one call
    assert stub.lib.calls == [("tonemap", 5, 6, tm, None)]
    m.EnableBloom(threshold=2.0, levels=3)
    assert m._tonemapped is None and stub.lib.calls == [("tonemap", 5, 6, tm, None)]
    assert m.ToneMap(destination=dest, operator="linear", exposure=0.5, white=2.0) is dest
    d = tuple(float(F(DEFAULTS[k])) for k in BLOOM_FIELDS[:5])
    assert stub.lib.calls[1:] == [("bloom", 5, 6, (2.0,) + d[1:] + (3, 0), None), ("tonemap", 6, 6, tm, None)]   # _converged is only read
    # with auto-exposure: metering, bloom and tone mapping share the state
    m._exposure, m._exposureState, m._temporal = {}, _StateTensor(ptr=0x9000), None
    del stub.lib.calls[:]
    m.ToneMap(destination=dest)
    assert stub.lib.calls == [("auto_exposure", 5, 0, 0x9000), ("bloom", 5, 6, (2.0,) + d[1:] + (3, 0), 0x9000),
                              ("tonemap", 6, 6, (1.0, 4.0, 2, 0), 0x9000)]
    m.DisableBloom()
    assert m._bloom is None
    del stub.lib.calls[:]
    m.ToneMap(destination=dest)
    assert stub.lib.calls == [("auto_exposure", 5, 0, 0x9000), ("tonemap", 5, 6, (1.0, 4.0, 2, 0), 0x9000)]
