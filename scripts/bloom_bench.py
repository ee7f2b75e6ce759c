"""Time of the bloom (include/urt.h urt_bloom, RayTraceMaster.EnableBloom) at 1920x1080 and 3840x2160, on a rendered C4 frame and on a
constant image of 4.0 (every texel above the threshold).

Cases, per size and content.  Device calls are timed with events on a stream the context issues on, after `--warmup` calls, over
`--iters` calls, in `--repeats` repeats (median and spread reported), the cases alternating within every repeat:
  copy            a device-to-device copy of one RGBA32F image (16 B read + 16 B written per texel): the rate the calls are held against;
  bloom_levels1   urt_bloom with levels = 1: the two kernels that touch the whole image (the prefiltering first downsample and the
                  composite) and nothing else;
  bloom           urt_bloom with the defaults (6 levels, 12 kernels);
  bloom_levels16  urt_bloom down to 1 x 1 (11 or 12 levels): what the tail of small launches costs;
  bloom_in_place  the defaults with dst == src;
  tonemap         urt_tonemap in place, for scale.
`bytes` is the compulsory traffic of a call: src read, dst written, and the pyramid written once and read once (32 B per pyramid texel);
`of_copy` is that traffic over the time, as a fraction of the same session's copy rate.  And, per size, on the C4 frame, with a host
clock around `--iters` calls that end with one synchronisation:
  master_tonemap / master_bloom_tonemap                  RayTraceMaster.ToneMap() without and with EnableBloom();
  master_metered_tonemap / master_metered_bloom_tonemap  the same with EnableAutoExposure().

`first_downsample` in every line is "staged", what the library runs; on an experiment build (URT_LIB_PATH=... URT_ALLOW_EXPERIMENT=1)
it is "direct": the A/B of the first downsample in profiles/r22_logs/ ran this script once per library, alternating in one session, the
second library built from this tree with profiles/r22_logs/bloom_direct_first.patch applied.

    python scripts/bloom_bench.py [--sizes 1920x1080,3840x2160] [--iters 50] [--repeats 5] [--json out.json]
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

from unityraytracer_amd import Context, RayTraceMaster, _lib, scenes  # noqa: E402
from unityraytracer_amd.unity_api import RenderTexture  # noqa: E402

F = np.float32


def summary(ms):
    med = float(np.median(ms))
    return {"ms": [round(v, 5) for v in ms], "ms_median": round(med, 5), "spread_pct": round(float((max(ms) - min(ms)) / med * 100), 2) if med > 0 else 0.0}


def pyramid_texels(w, h, levels):
    n = 0
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        n += w * h
        if w == 1 and h == 1:
            break
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    form = "direct" if _lib.load().urt_abi_version() < 0 else "staged"      # the only experiment build this script is run on
    results = []

    def emit(r):
        r = {"first_downsample": form, **r}
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
        constant.SetPixels(np.full((H, W, 4), 4.0, F))
        out = RenderTexture(ctx, W, H)
        scratch = RenderTexture(ctx, W, H)
        a_img, b_img = torch.ones((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        # ---- device calls, events on the stream the context issues on ----
        stream = torch.cuda.Stream(dev)                         # a real stream (torch's default one is handle 0 = "the library's own")
        torch.cuda.set_stream(stream)
        ctx.set_stream(stream.cuda_stream)
        tp = _lib.TonemapParams(1.0, 4.0, _lib.URT_TONEMAP_ACES, 0)

        def params(levels):
            d = _lib.BLOOM_DEFAULTS
            return _lib.BloomParams(d["threshold"], d["soft_knee"], d["clamp"], d["scatter"], d["intensity"], levels, 0)

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
            scratch.SetPixels(tex.GetPixels())                  # the in-place cases work on a copy

            def bloom(levels, src, dst):
                p = params(levels)
                return lambda: ctx.check(ctx.lib.urt_bloom(ctx._h, src.handle, dst.handle, C.byref(p), None))

            def traffic(levels):
                return 32 * n + 32 * pyramid_texels(W, H, levels)

            calls = {                                           # the raw entry points
                "copy": (lambda: b_img.copy_(a_img), 32 * n),
                "bloom_levels1": (bloom(1, tex, out), traffic(1)),
                "bloom": (bloom(6, tex, out), traffic(6)),
                "bloom_levels16": (bloom(16, tex, out), traffic(16)),
                "bloom_in_place": (bloom(6, scratch, scratch), traffic(6)),
                "tonemap": (lambda: ctx.check(ctx.lib.urt_tonemap(ctx._h, out.handle, out.handle, C.byref(tp), None)), 32 * n),
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
        ctx.set_stream(None)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))

        # ---- RayTraceMaster.ToneMap(), host clock, one synchronisation at the end of every repeat ----
        def master_case(metered, bloomed):
            (m.EnableAutoExposure if metered else m.DisableAutoExposure)()
            (m.EnableBloom if bloomed else m.DisableBloom)()
            for _ in range(args.warmup):
                m.ToneMap()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                m.ToneMap()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.iters

        steps = {"master_tonemap": (False, False), "master_bloom_tonemap": (False, True),
                 "master_metered_tonemap": (True, False), "master_metered_bloom_tonemap": (True, True)}
        ms = {c: [] for c in steps}
        for _ in range(args.repeats):
            for c, (metered, bloomed) in steps.items():
                ms[c].append(master_case(metered, bloomed))
        for c in steps:
            r = {"width": W, "height": H, "content": "c4_frame", "case": c, **summary(ms[c])}
            if "bloom" in c:
                r["bloom_cost_ms"] = round(r["ms_median"] - float(np.median(ms[c.replace("bloom_", "")])), 4)
            emit(r)
        for t in (constant, out, scratch):
            t.Release()
        m.OnDisable()
        ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
