"""Time of auto-exposure and tone mapping (include/urt.h urt_auto_exposure / urt_tonemap, RayTraceMaster.ToneMap) at 1920x1080 and
3840x2160, on a rendered C4 frame and on the constant image (every texel in one histogram bin: the worst case for the LDS adds).

Cases, per size and content.  Device calls are timed with events on a stream the context issues on, after `--warmup` calls, over
`--iters` calls, in `--repeats` repeats (median and spread reported), the cases alternating within every repeat:
  copy          a device-to-device copy of one RGBA32F image (16 B read + 16 B written per texel, urt_tonemap's own traffic): the rate
                the two calls are held against;
  auto_exposure urt_auto_exposure: the zeroing of the state, k_luminance_histogram and k_exposure_resolve; 16 B read per texel;
  auto_exposure_count  the same with a count texture, 32 B read per texel;
  tonemap       urt_tonemap (ACES, with the state) into a second texture; 32 B per texel;
and, per size, on the C4 frame, with a host clock around steps that end with the image in host memory:
  present_srgb8          (a) the RGBA8 sRGB formatted readback of _converged: what a host pays today for a clipped frame;
  tonemap_present_srgb8  (b) ToneMap() with auto-exposure, then the same readback of its result: (b) - (a) is the cost of ToneMap();
  readback_host_tonemap  (c) the RGBA32F readback of _converged, ACES in numpy (float32, the operator of include/urt.h) and the host sRGB
                         encoder: what a host does today for a tone-mapped frame.

    python scripts/tonemap_bench.py [--sizes 1920x1080,3840x2160] [--iters 100] [--repeats 5] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context, RayTraceMaster, _lib, host_io, scenes  # noqa: E402
from unityraytracer_amd.unity_api import RenderTexture  # noqa: E402

F = np.float32


def summary(ms):
    med = float(np.median(ms))
    return {"ms": [round(v, 5) for v in ms], "ms_median": round(med, 5), "spread_pct": round(float((max(ms) - min(ms)) / med * 100), 2) if med > 0 else 0.0}


def host_aces(rgba, exposure):
    """include/urt.h URT_TONEMAP_ACES on the host, float32."""
    x = rgba[..., :3] * F(exposure)
    x = np.where(x > 0, np.minimum(x, F(65504.0)), F(0.0)).astype(F)
    out = rgba.copy()
    out[..., :3] = np.minimum((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14)), F(1.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)

    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        n = W * H
        ctx = Context(0)
        m = RayTraceMaster(ctx, scenes.config4(W, H))
        for _ in range(args.frames):
            m.OnRenderImage()
        ctx.synchronize()
        constant = RenderTexture(ctx, W, H)
        constant.SetPixels(np.tile(np.array([0.5, 0.5, 0.5, 1.0], F), (H, W, 1)))
        ones = RenderTexture(ctx, W, H)
        ones.SetPixels(np.ones((H, W, 4), F))
        out = RenderTexture(ctx, W, H)
        state = torch.zeros(260, dtype=torch.int32, device=dev)
        a_img, b_img = torch.ones((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        # ---- device calls, events on the stream the context issues on ----
        stream = torch.cuda.Stream(dev)                         # a real stream (torch's default one is handle 0 = "the library's own")
        torch.cuda.set_stream(stream)
        ctx.set_stream(stream.cuda_stream)
        sp = C.c_void_p(state.data_ptr())
        ep, tp = _lib.ExposureParams(0.18, 1.0 / 64.0, 64.0, 1.0, 100, 950), _lib.TonemapParams(1.0, 4.0, _lib.URT_TONEMAP_ACES, 0)

        def timed(call):
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                call()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.iters

        for content, tex in (("c4_frame", m._converged), ("constant", constant)):
            calls = {                                           # the raw entry points: the Python wrappers wait for torch's stream, which is this one
                "copy": (lambda: b_img.copy_(a_img), 32 * n),
                "auto_exposure": (lambda: ctx.check(ctx.lib.urt_auto_exposure(ctx._h, tex.handle, 0, C.byref(ep), sp)), 16 * n),
                "auto_exposure_count": (lambda: ctx.check(ctx.lib.urt_auto_exposure(ctx._h, tex.handle, ones.handle, C.byref(ep), sp)), 32 * n),
                "tonemap": (lambda: ctx.check(ctx.lib.urt_tonemap(ctx._h, tex.handle, out.handle, C.byref(tp), sp)), 32 * n),
            }
            ms = {c: [] for c in calls}
            for _ in range(args.repeats):                       # alternate the cases within every repeat
                for c, (fn, _) in calls.items():
                    ms[c].append(timed(fn))
            copy_gbs = calls["copy"][1] / (float(np.median(ms["copy"])) * 1e-3) / 1e9
            for c, (_, nbytes) in calls.items():
                s = summary(ms[c])
                gbs = nbytes / (s["ms_median"] * 1e-3) / 1e9
                emit({"width": W, "height": H, "content": content, "case": c, **s, "bytes": nbytes, "GBps": round(gbs, 1),
                      "of_copy": round(gbs / copy_gbs, 3)})
            st = ctx.exposure_state(state)
            emit({"width": W, "height": H, "content": content, "case": "state", "exposure": st["exposure"], "counted": st["counted"],
                  "skipped": st["skipped"], "bins_used": int((st["hist"] > 0).sum()), "largest_bin_share": round(float(st["hist"].max()) / n, 4)})
        ctx.set_stream(None)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))

        # ---- per presented frame, host clock, the image in host memory at the end of every step ----
        m.EnableAutoExposure()
        m.ToneMap()
        ctx.synchronize()
        exposure = ctx.exposure_state(m._exposureState)["exposure"]

        def present(t):
            return t.ReadEnd(t.ReadBegin("RGBA8_SRGB"), copy=False)

        steps = {
            "present_srgb8": lambda: present(m._converged),
            "tonemap_present_srgb8": lambda: present(m.ToneMap()),
            "readback_host_tonemap": lambda: host_io.encode_srgb8(host_aces(m._converged.ReadEnd(m._converged.ReadBegin("RGBA32F"), copy=False), exposure)),
        }
        ms = {c: [] for c in steps}
        host_iters = max(3, args.iters // 10)
        for _ in range(args.repeats):
            for c, fn in steps.items():
                fn(); fn()
                t0 = time.perf_counter()
                for _ in range(host_iters):
                    fn()
                ms[c].append((time.perf_counter() - t0) * 1e3 / host_iters)
        same = np.array_equal(steps["tonemap_present_srgb8"]()[..., :3], steps["readback_host_tonemap"]()[..., :3])
        base = float(np.median(ms["present_srgb8"]))
        for c in steps:
            r = {"width": W, "height": H, "content": "c4_frame", "case": c, **summary(ms[c])}
            if c == "tonemap_present_srgb8":
                r["tonemap_cost_ms"] = round(r["ms_median"] - base, 4)
                r["same_bytes_as_host_path"] = bool(same)
            emit(r)
        for t in (constant, ones, out):
            t.Release()
        m.OnDisable()
        ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
