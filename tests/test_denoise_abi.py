"""CPU: the denoiser entry point (include/urt.h urt_denoise) — the header compiles as C99, urt_DenoiseParams has one layout in gcc, ctypes
and the C# binding, the defaults agree, the symbol is exported, Context.denoise and RayTraceMaster.Denoise validate their arguments
before they call the library, and the float64 reference (tests/denoise_ref.py) passes its own sanity checks, among them rule 1's clause
on the demodulated colour and the containment and scale invariance that tests/test_gpu_denoise_range.py asks of the library."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from denoise_ref import H, MAX_COLOR, demodulator, denoise_ref, reach, surface_mask, window_min_max
from unityraytracer_amd import RayTraceMaster, _lib, unity_api
from unityraytracer_amd._lib import UrtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URT_H = os.path.join(ROOT, "include", "urt.h")
FIELDS = ("iterations", "sigma_color", "sigma_normal", "sigma_depth")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(tmp_path):
    inc = ["-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    decl = tmp_path / "decl.c"                  # the prototype, compiled only (the symbol lives in the HIP library)
    decl.write_text('#include "urt.h"\n'
                    'int (*fn)(urt_context*, urt_handle, urt_handle, urt_handle, urt_handle, urt_handle, const urt_DenoiseParams*) = urt_denoise;\n')
    subprocess.run(["gcc", *inc, "-c", str(decl), "-o", str(tmp_path / "decl.o")], check=True)
    src = tmp_path / "layout.c"
    src.write_text('#include "urt.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(void) {\n'
                   '  urt_DenoiseParams d = {URT_DENOISE_DEFAULT_ITERATIONS, URT_DENOISE_DEFAULT_SIGMA_COLOR, URT_DENOISE_DEFAULT_SIGMA_NORMAL,\n'
                   '                         URT_DENOISE_DEFAULT_SIGMA_DEPTH};\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(urt_DenoiseParams), offsetof(urt_DenoiseParams, iterations),\n'
                   '         offsetof(urt_DenoiseParams, sigma_color), offsetof(urt_DenoiseParams, sigma_normal),\n'
                   '         offsetof(urt_DenoiseParams, sigma_depth));\n'
                   '  printf("%d %a %a %a\\n", d.iterations, d.sigma_color, d.sigma_normal, d.sigma_depth);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", *inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size, *offs = (int(v) for v in out[0].split())
    assert size == C.sizeof(_lib.DenoiseParams) == 16
    assert offs == [getattr(_lib.DenoiseParams, f).offset for f in FIELDS] == [0, 4, 8, 12]
    it, sc, sn, sz = out[1].split()
    assert {"iterations": int(it), "sigma_color": float.fromhex(sc), "sigma_normal": float.fromhex(sn),
            "sigma_depth": float.fromhex(sz)} == \
        {k: (v if k == "iterations" else float(np.float32(v))) for k, v in _lib.DENOISE_DEFAULTS.items()}


def test_declarations_agree_across_header_lib_and_csharp():
    text = open(URT_H).read()
    assert re.search(r"URT_API int urt_denoise\(urt_context\* ctx, urt_handle src, urt_handle dst, urt_handle hit, urt_handle normal, "
                     r"urt_handle albedo,\s+const urt_DenoiseParams\* params\);", text)
    body = re.search(r"typedef struct urt_DenoiseParams \{(.*?)\} urt_DenoiseParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(int32_t|float) (\w+);", body, re.M) == [("int32_t", "iterations"), ("float", "sigma_color"),
                                                                     ("float", "sigma_normal"), ("float", "sigma_depth")]
    assert "urt_denoise" in _lib.ABI_SYMBOLS
    cs = open(os.path.join(ROOT, "integration", "UrtNative.cs")).read()
    assert re.search(r"\[DllImport\(Lib\)\] internal static extern int urt_denoise\(IntPtr ctx, ulong src, ulong dst, ulong hit, "
                     r"ulong normal, ulong albedo, in DenoiseParams p\);", cs)
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*internal struct DenoiseParams \{(.*?)\}", cs, re.S)
    assert m, "the C# DenoiseParams struct is missing"
    assert re.findall(r"public (int|float) (\w+);", m.group(1)) == [("int", "iterations"), ("float", "sigmaColor"), ("float", "sigmaNormal"),
                                                                  ("float", "sigmaDepth")]
    for name, v in _lib.DENOISE_DEFAULTS.items():
        macro = {"iterations": "ITERATIONS", "sigma_color": "SIGMA_COLOR", "sigma_normal": "SIGMA_NORMAL", "sigma_depth": "SIGMA_DEPTH"}[name]
        hv = re.search(rf"#define URT_DENOISE_DEFAULT_{macro} ([0-9.]+)f?\b", text).group(1)
        assert float(hv) == v, name


def test_reference_defaults_are_the_documented_ones():
    import inspect
    sig = inspect.signature(denoise_ref).parameters
    assert {k: sig[k].default for k in FIELDS} == _lib.DENOISE_DEFAULTS
    cs = open(os.path.join(ROOT, "integration", "UrtUnityShim.cs")).read()
    d = _lib.DENOISE_DEFAULTS
    assert (f"int iterations = {d['iterations']}, float sigmaColor = {d['sigma_color']}f, float sigmaNormal = {d['sigma_normal']}f, "
            f"float sigmaDepth = {d['sigma_depth']}f") in cs


def test_symbol_is_exported(built_library):
    lib = C.CDLL(built_library)
    assert hasattr(lib, "urt_denoise")
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", built_library], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT urt_denoise\b", out)


def test_null_context_is_rejected(built_library):
    lib = _lib.load()
    assert lib.urt_denoise(None, 1, 2, 3, 4, 0, None) == 1        # URT_ERR_INVALID_ARGUMENT, no device needed


# ---- the Python wrappers, on a stub library ------------------------------------------------------------------------------------------
class _StubLib:
    """Records the calls Context.denoise makes instead of reaching a GPU."""

    def __init__(self):
        self.calls = []

    def urt_denoise(self, *a):
        self.calls.append(("denoise",) + a[1:6] + (tuple(getattr(a[6]._obj, f) for f in FIELDS),))
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


def stub_textures(ctx):
    return {k: stub_texture(ctx, v) for k, v in (("src", 11), ("dst", 12), ("hit", 13), ("normal", 14), ("albedo", 15))}


BAD_CALLS = {
    "src_not_a_texture": (TypeError, {"src": 7}),
    "hit_none": (TypeError, {"hit": None}),
    "albedo_numpy": (TypeError, {"albedo": np.zeros((3, 4, 4), np.float32)}),
    "other_context": (ValueError, {"normal": "other"}),
    "released": (ValueError, {"dst": "released"}),
    "size": (ValueError, {"albedo": "small"}),
    "dst_is_guide": (ValueError, {"dst": "hit"}),
    "iterations_0": (ValueError, {"iterations": 0}),
    "iterations_6": (ValueError, {"iterations": 6}),
    "iterations_float": (TypeError, {"iterations": 2.0}),
    "iterations_bool": (TypeError, {"iterations": True}),
    "sigma_nan": (ValueError, {"sigma_normal": float("nan")}),
    "sigma_str": (TypeError, {"sigma_color": "1"}),
}


def _resolve(ctx, tex, kw):
    out = dict(kw)
    for k, v in kw.items():
        if not isinstance(v, str):
            continue
        if v == "other":
            out[k] = stub_texture(stub_context(), 99)
        elif v == "released":
            out[k] = stub_texture(ctx, 0)
        elif v == "small":
            out[k] = stub_texture(ctx, 98, w=3)
        elif v == "hit":
            out[k] = tex["hit"]
    return out


@pytest.mark.parametrize("case", sorted(BAD_CALLS))
def test_context_denoise_validates_before_calling_the_library(case):
    ctx = stub_context()
    tex = stub_textures(ctx)
    exc, kw = BAD_CALLS[case]
    with pytest.raises(exc):
        ctx.denoise(**{**tex, **_resolve(ctx, tex, kw)})
    assert ctx.lib.calls == []


def test_context_denoise_passes_handles_and_params():
    ctx = stub_context()
    tex = stub_textures(ctx)
    ctx.denoise(**tex)
    ctx.denoise(tex["src"], tex["src"], tex["hit"], tex["normal"], iterations=np.int64(2), sigma_color=0, sigma_normal=np.float32(0.25),
                sigma_depth=-1.0)
    d = _lib.DENOISE_DEFAULTS
    assert ctx.lib.calls == [("denoise", 11, 12, 13, 14, 15, (d["iterations"], np.float32(d["sigma_color"]), np.float32(d["sigma_normal"]),
                                                              np.float32(d["sigma_depth"]))),
                             ("denoise", 11, 11, 13, 14, 0, (2, 0.0, 0.25, -1.0))]


def test_denoise_arrays_rejects_bad_shapes():
    ctx = stub_context()
    img = np.zeros((3, 4, 4), np.float32)
    for args in ((np.zeros((3, 4, 3), np.float32), img, img), (img, np.zeros((4, 3, 4), np.float32), img),
                 (img, img, img, np.zeros((3, 4), np.float32))):
        with pytest.raises(ValueError):
            ctx.denoise_arrays(*args)
    assert ctx.lib.calls == []


def _stub_master(ctx, with_image=True):
    m = object.__new__(RayTraceMaster)
    m.ctx = ctx
    m._aov = m._denoised = None
    m._converged = stub_texture(ctx, 21) if with_image else None
    m.screen_width, m.screen_height = 4, 3
    return m


@pytest.mark.parametrize("case", ["no_image", "destination_numpy", "destination_other_context", "destination_released", "iterations",
                                  "sigma_nan", "unknown_param"])
def test_master_denoise_validates_before_calling_the_library(case):
    ctx = stub_context()
    m = _stub_master(ctx, with_image=case != "no_image")
    exc, kw = {
        "no_image": (UrtError, {}),
        "destination_numpy": (TypeError, {"destination": np.zeros((3, 4, 4), np.float32)}),
        "destination_other_context": (ValueError, {"destination": stub_texture(stub_context(), 5)}),
        "destination_released": (ValueError, {"destination": stub_texture(ctx, 0)}),
        "iterations": (ValueError, {"iterations": 9}),
        "sigma_nan": (ValueError, {"sigma_depth": float("nan")}),
        "unknown_param": (TypeError, {"sigma": 1.0}),
    }[case]
    with pytest.raises(exc):
        m.Denoise(**kw)
    assert ctx.lib.calls == []


def test_master_denoise_uses_its_feature_buffers():
    ctx = stub_context()
    m = _stub_master(ctx)
    m._aov = tuple(stub_texture(ctx, h) for h in (31, 32, 33, 34))
    dst = stub_texture(ctx, 40)
    assert m.Denoise(dst, iterations=3) is dst
    assert ctx.lib.calls == [("denoise", 21, 40, 31, 32, 33, (3, np.float32(_lib.DENOISE_DEFAULTS["sigma_color"]),
                                                              np.float32(_lib.DENOISE_DEFAULTS["sigma_normal"]),
                                                              np.float32(_lib.DENOISE_DEFAULTS["sigma_depth"])))]


# ---- the float64 reference on its own --------------------------------------------------------------------------------------------------
def _guides(rng, h, w, miss=0.0):
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normal = np.concatenate([n, np.full((h, w, 1), 3.0)], -1).astype(np.float32)
    hit = np.concatenate([rng.uniform(-5, 5, (h, w, 3)), rng.uniform(1, 20, (h, w, 1))], -1).astype(np.float32)
    m = rng.random((h, w)) < miss
    normal[m] = 0.0
    hit[m] = (0, 0, 0, np.inf)
    return hit, normal


def test_reference_keeps_a_constant_image_constant():
    rng = np.random.default_rng(1)
    hit, normal = _guides(rng, 23, 31, miss=0.1)
    color = np.empty((23, 31, 4), np.float32)
    color[...] = (0.25, 3.0, 0.5, 0.75)
    albedo = np.concatenate([rng.uniform(0, 1, (23, 31, 3)), np.zeros((23, 31, 1))], -1).astype(np.float32)
    for alb in (None, albedo):
        out = denoise_ref(color, hit, normal, alb, iterations=5, sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.2)
        surf = surface_mask(color, hit, normal)
        if alb is None:
            np.testing.assert_allclose(out[surf], np.broadcast_to(color[0, 0], out[surf].shape), rtol=1e-12)
        else:                       # demodulated, it is no longer constant; with the colour term off it is (c / d) blurred, times d
            out = denoise_ref(color, hit, normal, alb, iterations=2, sigma_color=0, sigma_normal=0, sigma_depth=0)
            np.testing.assert_allclose(out[..., 3], color[..., 3])
        np.testing.assert_array_equal(out[~surf], color[~surf])


def _b3_blur_skipped_borders(img, valid):
    """One pass with every sigma off: a normalised separable convolution with the B3-spline kernel, zero outside the image and at the
    pass-through pixels (numpy.convolve along each axis, not the shift-and-add of the reference)."""
    k = np.array(H)

    def sep(a):
        a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, a)
        return np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, a)

    num = np.stack([sep(img[..., ch] * valid) for ch in range(3)], -1)
    den = sep(valid.astype(np.float64))
    return num / den[..., None]


def test_reference_one_pass_without_sigmas_is_a_b3_spline_blur():
    rng = np.random.default_rng(2)
    h, w = 19, 27
    hit, normal = _guides(rng, h, w, miss=0.15)
    color = rng.uniform(0, 10, (h, w, 4)).astype(np.float32)
    out = denoise_ref(color, hit, normal, None, iterations=1, sigma_color=0, sigma_normal=-1, sigma_depth=0)
    surf = surface_mask(color, hit, normal)
    ref = _b3_blur_skipped_borders(color[..., :3].astype(np.float64), surf)
    np.testing.assert_allclose(out[..., :3][surf], ref[surf], rtol=1e-12)
    np.testing.assert_array_equal(out[~surf], color[~surf])


def test_reference_pass_through_rules():
    rng = np.random.default_rng(3)
    hit, normal = _guides(rng, 4, 5)
    color = rng.uniform(0, 1, (4, 5, 4)).astype(np.float32)
    normal[0, 0, 3] = 0                         # kind 0
    hit[0, 1, 3] = np.inf                       # depth not finite
    hit[0, 2, 3] = -1                           # depth <= 0
    color[0, 3, 1] = np.nan                     # colour not finite
    normal[0, 4, 2] = np.inf                    # normal not finite
    surf = surface_mask(color, hit, normal)
    assert not surf[0].any() and surf[1:].all()


def test_reference_passes_through_an_overflowing_demodulated_colour():
    """Rule 1 on the float32 quotient c / d: not finite, or above 2^120 in magnitude."""
    rng = np.random.default_rng(4)
    hit, normal = _guides(rng, 3, 8)
    color = rng.uniform(0, 1, (3, 8, 4)).astype(np.float32)
    albedo = np.full((3, 8, 4), 0.5, np.float32)
    above = np.nextafter(MAX_COLOR, np.float32(np.inf))
    color[0, 0, 0], albedo[0, 0, 0] = 1e36, 0.0             # finite over the 1e-3 floor: inf
    color[0, 1, 1], albedo[0, 1, 1] = 1e36, np.nan          # a NaN albedo channel is 1e-3 too
    color[0, 2, 2], albedo[0, 2, 2] = -3e38, 0.5            # -inf
    color[0, 3, 0], albedo[0, 3, 0] = MAX_COLOR, 0.99       # finite, above 2^120
    color[0, 4, 1], albedo[0, 4, 1] = -above, 1.0           # the first float past -2^120
    color[0, 5, 2], albedo[0, 5, 2] = above, 8.0            # above 2^120 itself, but its quotient is not
    color[0, 6, 0], albedo[0, 6, 0] = MAX_COLOR, 1.0        # 2^120 exactly is filtered
    color[0, 7, 1], albedo[0, 7, 1] = -MAX_COLOR, 2.0
    surf = surface_mask(color, hit, normal, albedo)
    assert surf[0].tolist() == [False] * 5 + [True] * 3 and surf[1:].all()
    plain = surface_mask(color, hit, normal)                # without albedo the quotient is the colour
    assert plain[0].tolist() == [True, True, False, True, False, False, True, True] and plain[1:].all()
    for alb, mask in ((albedo, surf), (None, plain)):
        out = denoise_ref(color, hit, normal, alb, iterations=3, sigma_color=0, sigma_normal=0, sigma_depth=0)
        np.testing.assert_array_equal(out[~mask], color[~mask])
        assert np.isfinite(out).all() and (out[mask][:, :3] != color[mask][:, :3]).any(-1).all()


def test_reference_survives_one_overflowing_texel():
    """One texel of colour 1e36 over albedo 0 in a 67 x 33 all-surface image: the formula is finite and float32-representable at
    every pixel, and equals the formula of the image with that pixel's kind set to 0."""
    rng = np.random.default_rng(6)
    h, w = 33, 67
    hit, normal = _guides(rng, h, w)
    color = (10.0 ** rng.uniform(-3, 3, (h, w, 4))).astype(np.float32)
    albedo = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
    color[h // 2, w // 2, :3], albedo[h // 2, w // 2, :3] = 1e36, 0.0
    out = denoise_ref(color, hit, normal, albedo)
    assert np.isfinite(out.astype(np.float32)).all()
    masked = normal.copy()
    masked[h // 2, w // 2, 3] = 0
    np.testing.assert_array_equal(out, denoise_ref(color, hit, masked, albedo))
    np.testing.assert_array_equal(out[h // 2, w // 2], color[h // 2, w // 2])


@pytest.mark.parametrize("sig", ["all", "none", "color_1e-30", "color_1e38"])
def test_formula_stays_within_the_hull_of_its_reach(sig):
    """Property B of tests/test_gpu_denoise_range.py is a property of the formula: over the whole finite float range every filtered
    value lies in [min, max] of the demodulated colours of the surface pixels within reach (float64: 125 roundings of 2^-53)."""
    from test_gpu_denoise_range import B_SIGMAS, range_inputs
    w, h = 41, 29
    for it in (1, 5):
        color, hit, normal, albedo = range_inputs(10 * w + it, w, h)
        for alb in (None, albedo):
            surf = surface_mask(color, hit, normal, alb)
            s3 = np.broadcast_to(surf[..., None], (h, w, 3))
            assert 0.5 * h * w < surf.sum() < h * w
            d = demodulator(alb, color.shape).astype(np.float64)
            out = denoise_ref(color, hit, normal, alb, iterations=it, **B_SIGMAS[sig])
            np.testing.assert_array_equal(out[~surf], color[~surf])
            with np.errstate(all="ignore"):
                lo, hi = window_min_max(color[..., :3].astype(np.float64) / d, surf, reach(it))
            slack = 1e-12 * np.maximum(np.abs(lo), np.abs(hi))
            g = out[..., :3] / d
            assert np.isfinite(g[s3]).all() and ((g >= lo - slack) & (g <= hi + slack))[s3].all()


@pytest.mark.parametrize("k", [-40, -8, 8, 40])
def test_formula_is_invariant_under_powers_of_two(k):
    """Property C of tests/test_gpu_denoise_range.py is a property of the formula: colour and sigma_color times 2^k scale the result by
    2^k, depth times 2^k leaves it alone (to 1e-12 relative)."""
    from test_gpu_denoise_range import invariance_inputs
    w, h = 41, 29
    color, hit, normal, albedo = invariance_inputs(31 * w + k, w, h)
    sig = dict(sigma_color=50.0, sigma_normal=0.5, sigma_depth=0.3)
    c_scaled, z_scaled = color.copy(), hit.copy()
    c_scaled[..., :3] = np.ldexp(color[..., :3], k)
    z_scaled[..., 3] = np.ldexp(hit[..., 3], k)
    for alb in (None, albedo):
        surf = surface_mask(color, hit, normal, alb)
        base = denoise_ref(color, hit, normal, alb, **sig)[..., :3][surf]
        got = denoise_ref(c_scaled, hit, normal, alb, **dict(sig, sigma_color=50.0 * 2.0 ** k))[..., :3][surf]
        np.testing.assert_allclose(got, base * 2.0 ** k, rtol=1e-12, atol=0)
        got = denoise_ref(color, z_scaled, normal, alb, **sig)[..., :3][surf]
        np.testing.assert_allclose(got, base, rtol=1e-12, atol=0)
