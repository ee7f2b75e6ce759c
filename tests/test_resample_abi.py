"""CPU: the resampling entry points (include/urt.h urt_select_pixels, urt_blend_samples, urt_resample_below) — the declarations agree
across the header, the ctypes binding and the C# binding, the symbols are exported, a NULL context is rejected without a device and
nothing is returned, the Python wrappers validate their arguments before they call the library, and the float32 restatements
(tests/resample_ref.py) pass their own checks: a blend of weight 1 over every pixel is blit_add_history_ref bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from reproject_ref import blit_add_history_ref
from resample_ref import blend_samples_ref, select_pixels_ref
from unityraytracer_amd import RayTraceMaster, UrtError, _lib, unity_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("urt_select_pixels", "urt_blend_samples", "urt_resample_below")


def test_declarations_agree_across_header_lib_and_csharp():
    text = open(os.path.join(ROOT, "include", "urt.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert "URT_API int urt_select_pixels(urt_context* ctx, urt_handle count, float below, void* d_pixels, int capacity, int* out_n);" in flat
    assert ("URT_API int urt_blend_samples(urt_context* ctx, const void* d_pixels, const void* d_samples, int n, float weight, "
            "urt_handle dst, urt_handle count, float max_history);") in flat
    assert ("URT_API int urt_resample_below(urt_context* ctx, urt_handle dst, urt_handle count, float below, int samples, int bounces, "
            "float weight, float max_history, int* out_n);") in flat
    assert text.index("---- temporal reprojection") < text.index("---- resampling") < text.index("---- measurement")
    assert set(NAMES) <= set(_lib.ABI_SYMBOLS)
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    for name in NAMES:
        assert re.search(rf"\[DllImport\(Lib\)\] internal static extern int {name}\(IntPtr ctx, ", cs), name
    assert "ResampleDisocclusions" in open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()


def test_chunk_constant_is_the_kernels():
    text = open(os.path.join(ROOT, "unityraytracer_amd", "csrc", "resample.h")).read()
    rounds = int(re.search(r"constexpr int kSelectRounds = (\d+);", text).group(1))
    assert re.search(r"constexpr int kSelectChunk = 4 \* 64 \* kSelectRounds;", text)
    assert unity_api.SELECT_CHUNK == 4 * 64 * rounds


def test_symbols_are_exported(built_library):
    lib = C.CDLL(built_library)
    for name in NAMES:
        assert hasattr(lib, name), name
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(rf"\bT {name}\b", out), name


def test_null_context_is_rejected_and_nothing_is_returned(built_library):
    lib = _lib.load()
    n = C.c_int(-7)
    assert lib.urt_select_pixels(None, 1, 1.0, None, 0, C.byref(n)) == 1      # URT_ERR_INVALID_ARGUMENT, no device needed
    assert lib.urt_blend_samples(None, None, None, 0, 1.0, 1, 2, 0.0) == 1
    assert lib.urt_resample_below(None, 1, 2, 1.0, 1, 1, 1.0, 0.0, C.byref(n)) == 1
    assert n.value == -7


def test_without_a_device_the_calls_fail_loudly(built_library):
    if not torch.cuda.is_available():
        with pytest.raises(UrtError) as e:
            unity_api.Context(0)                                              # no context: no select_pixels / blend_samples / resample_below
        assert e.value.code == 3
    m = object.__new__(RayTraceMaster)                                        # and the master returns no count without its textures
    m._temporal = None
    with pytest.raises(UrtError):
        m.ResampleDisocclusions()


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return 0
        return call


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


def _tex(ctx, kind):
    if not isinstance(kind, str):
        return kind
    if kind == "other":
        return stub_texture(stub_context(), 99)
    if kind == "released":
        return stub_texture(ctx, 0)
    if kind == "small":
        return stub_texture(ctx, 98, 2, 2)
    return kind


SELECT_BAD = {
    "count_int": (TypeError, {"count": 3}),
    "count_numpy": (TypeError, {"count": np.zeros((3, 4, 4), F)}),
    "count_other_context": (ValueError, {"count": "other"}),
    "count_released": (ValueError, {"count": "released"}),
    "below_nan": (ValueError, {"below": float("nan")}),
    "below_str": (TypeError, {"below": "1"}),
    "below_bool": (TypeError, {"below": True}),
}


@pytest.mark.parametrize("case", sorted(SELECT_BAD))
def test_select_wrapper_rejects_bad_arguments_before_the_library(case):
    exc, change = SELECT_BAD[case]
    ctx = stub_context()
    kw = {"count": stub_texture(ctx, 1), "below": 1.0}
    kw.update({k: _tex(ctx, v) for k, v in change.items()})
    with pytest.raises(exc):
        ctx.select_pixels(**kw)
    assert ctx.lib.calls == []


BLEND_BAD = {
    "xy_numpy": (TypeError, {"xy": np.zeros((5, 2), np.int32)}),
    "xy_dtype": (TypeError, {"xy": torch.zeros((5, 2), dtype=torch.int64)}),
    "xy_shape": (ValueError, {"xy": torch.zeros((5, 3), dtype=torch.int32)}),
    "xy_flat": (ValueError, {"xy": torch.zeros(10, dtype=torch.int32)}),
    "samples_dtype": (TypeError, {"samples": torch.zeros((5, 4), dtype=torch.float64)}),
    "samples_shape": (ValueError, {"samples": torch.zeros((5, 3), dtype=torch.float32)}),
    "samples_list": (TypeError, {"samples": [[0.0] * 4] * 5}),
    "not_on_the_device": (ValueError, {}),                                    # well-formed CPU tensors
    "dst_int": (TypeError, {"dst": 4}),
    "count_none": (TypeError, {"count": None}),
    "dst_other_context": (ValueError, {"dst": "other"}),
    "count_released": (ValueError, {"count": "released"}),
    "count_size": (ValueError, {"count": "small"}),
    "dst_is_count": (ValueError, {"count": "dst"}),
    "weight_zero": (ValueError, {"weight": 0.0}),
    "weight_negative": (ValueError, {"weight": -1.0}),
    "weight_inf": (ValueError, {"weight": float("inf")}),
    "weight_nan": (ValueError, {"weight": float("nan")}),
    "weight_str": (TypeError, {"weight": "1"}),
    "max_history_half": (ValueError, {"max_history": 0.5}),
    "max_history_negative": (ValueError, {"max_history": -1.0}),
    "max_history_nan": (ValueError, {"max_history": float("nan")}),
}


@pytest.mark.parametrize("case", sorted(BLEND_BAD))
def test_blend_wrapper_rejects_bad_arguments_before_the_library(case):
    exc, change = BLEND_BAD[case]
    ctx = stub_context()
    kw = {"xy": torch.zeros((5, 2), dtype=torch.int32), "samples": torch.zeros((5, 4), dtype=torch.float32),
          "dst": stub_texture(ctx, 1), "count": stub_texture(ctx, 2)}
    for k, v in change.items():
        kw[k] = kw["dst"] if isinstance(v, str) and v == "dst" else _tex(ctx, v)
    with pytest.raises(exc):
        ctx.blend_samples(**kw)
    assert ctx.lib.calls == []


RESAMPLE_BAD = {
    "dst_int": (TypeError, {"dst": 4}),
    "count_other_context": (ValueError, {"count": "other"}),
    "count_size": (ValueError, {"count": "small"}),
    "dst_is_count": (ValueError, {"count": "dst"}),
    "below_nan": (ValueError, {"below": float("nan")}),
    "samples_zero": (ValueError, {"samples": 0}),
    "samples_float": (TypeError, {"samples": 1.0}),
    "bounces_65": (ValueError, {"bounces": 65}),
    "weight_zero": (ValueError, {"weight": 0}),
    "max_history_quarter": (ValueError, {"max_history": 0.25}),
}


@pytest.mark.parametrize("case", sorted(RESAMPLE_BAD))
def test_resample_wrapper_rejects_bad_arguments_before_the_library(case):
    exc, change = RESAMPLE_BAD[case]
    ctx = stub_context()
    kw = {"dst": stub_texture(ctx, 1), "count": stub_texture(ctx, 2), "below": 1.0, "samples": 1, "bounces": 2}
    for k, v in change.items():
        kw[k] = kw["dst"] if isinstance(v, str) and v == "dst" else _tex(ctx, v)
    with pytest.raises(exc):
        ctx.resample_below(**kw)
    assert ctx.lib.calls == []
    good = {"dst": stub_texture(ctx, 1), "count": stub_texture(ctx, 2), "below": 4.5, "samples": 2, "bounces": 0, "weight": 0.5, "max_history": 8}
    ctx.resample_below(**good)
    assert ctx.lib.calls == ["urt_resample_below"]


def test_master_refuses_without_temporal_accumulation_or_an_image():
    m = object.__new__(RayTraceMaster)
    m._temporal = None
    with pytest.raises(UrtError):
        m.ResampleDisocclusions()
    m._temporal = {"max_history": 64.0}
    m._converged = m._tcount = None
    m._currentSample = 0
    with pytest.raises(UrtError):
        m.ResampleDisocclusions()


# ---- the restatements' own checks ----------------------------------------------------------------------------------------------------
def test_select_reference_on_hand_written_cases():
    nan, inf = float("nan"), float("inf")
    c = np.array([[0.0, 1.0, 2.0], [nan, -1.0, inf]], F)                       # 3 x 2, row 0 = bottom
    assert select_pixels_ref(c, 1.0).tolist() == [[0, 0], [0, 1], [1, 1]]      # 0 < 1; NaN and negative are selected, +inf is not
    assert select_pixels_ref(c, 2.0).tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]]
    assert select_pixels_ref(c, inf).tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1]]
    assert select_pixels_ref(c, -inf).tolist() == [[0, 1]]                     # only NaN fails count >= -inf
    c4 = np.zeros((2, 3, 4), F)
    c4[..., 0] = c
    c4[..., 1:] = -5.0                                                         # only .x counts
    assert select_pixels_ref(c4, 1.0).tolist() == [[0, 0], [0, 1], [1, 1]]
    full = np.full((2, 3), -inf, F)
    assert select_pixels_ref(full, 0.0).tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]]
    r = select_pixels_ref(np.ones((2, 3), F), 1.0)
    assert r.shape == (0, 2) and r.dtype == np.int32


@pytest.mark.parametrize("max_history", [0.0, 1.0, 8.0])
def test_blend_reference_of_weight_one_is_blit_add_history(max_history):
    h, w = 17, 23
    rng = np.random.default_rng(11)
    src = rng.uniform(0, 2, (h, w, 4)).astype(F)
    dst = rng.uniform(0, 2, (h, w, 4)).astype(F)
    count = rng.uniform(0, 20, (h, w, 4)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1.0, 7.0, 8.0, 9.0, 200.0, 0.5], F)
    count.reshape(-1, 4)[: 4 * len(special), 0] = np.tile(special, 4)
    X, Y = np.meshgrid(np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32))
    xy = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
    got, cnt = blend_samples_ref(xy, src.reshape(-1, 4), dst, count, 1.0, max_history)
    ref, rcnt = blit_add_history_ref(src, dst, count, max_history)
    assert got.view(np.uint32).tobytes() == ref.view(np.uint32).tobytes()
    assert cnt.view(np.uint32).tobytes() == rcnt.view(np.uint32).tobytes()
    perm = rng.permutation(len(xy))                                            # the order of a list of distinct pixels does not matter
    got2, cnt2 = blend_samples_ref(xy[perm], src.reshape(-1, 4)[perm], dst, count, 1.0, max_history)
    assert got2.tobytes() == got.tobytes() and cnt2.tobytes() == cnt.tobytes()


def test_blend_reference_weights_and_skips():
    dst = np.full((2, 3, 4), 2.0, F)
    count = np.zeros((2, 3, 4), F)
    count[..., 0] = [[0.0, 3.0, 100.0], [np.nan, -2.0, 6.0]]
    xy = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [0, -1], [1, 1]], np.int32)  # (3, 0) and (0, -1) lie outside
    t = np.full((6, 4), 4.0, F)
    out, cnt = blend_samples_ref(xy, t, dst, count, weight=2.0, max_history=8.0)
    assert cnt[..., 0].tolist()[0] == [2.0, 5.0, 8.0]                          # s = 0, 3, min(100, 8 - 2)
    assert np.isnan(cnt[1, 0, 0]) and cnt[1, 1, 0] == 2.0 and cnt[1, 2, 0] == 6.0   # (0, 1) and (2, 1) are not in the list; (1, 1): s = 0
    assert out[0, 0].tolist() == [4.0, 4.0, 4.0, 1.0]                          # a = 1: the sample, alpha a * a
    a = F(2.0) / F(5.0)
    assert out[0, 1, 0] == F(4.0) * a + F(2.0) * (F(1.0) - a)
    assert (out[1, 0] == 2.0).all() and (out[1, 2] == 2.0).all()
    out2, cnt2 = blend_samples_ref(xy, t, dst, count, weight=0.5, max_history=0.0)
    assert cnt2[0, 2, 0] == 100.5 and cnt2[0, 0, 0] == 0.5
    with pytest.raises(AssertionError):
        blend_samples_ref(np.array([[1, 1], [1, 1]], np.int32), t[:2], dst, count)
