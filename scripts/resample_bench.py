"""Time of the resampling step (include/urt.h urt_select_pixels, urt_resample_below) next to the host route a caller had before it, on
C3 at 1920x1080 and 3840x2160: four frames with temporal accumulation, then the 3 degree yaw of
tests/test_gpu_radiance_query.py::test_resample_pixels_of_a_disocclusion_mask, which leaves a few per cent of the pixels with count 0.

  (a) select       urt_select_pixels(count, 1.0) into a list of the selected size (three launches and one synchronisation per call) and,
                   in the same repeat, urt_blit of a texture of the same size: the blit reads and writes the image once, the selection
                   reads it twice — the same bytes, so the blit is the yardstick.  `select_count_only` is the capacity-0 form.
  (b) resample     urt_resample_below(converged, count, 1.0, numRays, numBounces, 1, max_history) end to end.  A call changes the counts
                   it selected, so every timed call is preceded by a urt_blit that restores the count texture; the same blit is timed
                   alone in the same repeat and subtracted (`ms` is the difference, `ms_pair` and `ms_restore` are what was measured).
                   `resample_wall` is the same call in host wall time (restore untimed), for the comparison with (c).
  (c) host_route   what a caller does without these entry points, in host wall time: GetPixels of the count texture and of the image,
                   np.nonzero, RayTraceMaster.ResamplePixels (host form), the blend of the header in numpy over the selected pixels,
                   SetPixels of the image and of the count texture.

(a) and (b): device events on a torch stream the context is set to issue on, `--warmup` calls, then `--iters` timed calls, `--repeats`
times; median and spread of the repeats; the forms alternate inside every repeat.  (c) and resample_wall: time.perf_counter around the
calls and a synchronisation, `--wall-iters` calls per repeat.  One JSON line per (size, form); --json writes them all.

    python scripts/resample_bench.py [--sizes 1080p,2160p] [--iters 20] [--warmup 5] [--repeats 5] [--wall-iters 3] [--json out.json]
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

from unityraytracer_amd import Context, RayTraceMaster, scenes  # noqa: E402
from unityraytracer_amd.unity_api import RenderTexture  # noqa: E402

SIZES = {"1080p": (1920, 1080), "2160p": (3840, 2160)}
F = np.float32


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def report(results, size, form, ms, **extra):
    med = float(np.median(ms))
    r = {"size": size, "form": form, "ms": [round(x, 4) for x in ms], "ms_median": med,
         "spread_pct": float((max(ms) - min(ms)) / med * 100) if med > 0 else 0.0, **extra}
    print(json.dumps(r), flush=True)
    results.append(r)


def host_blend(conv, cnt, ys, xs, t, max_history):
    """urt_blend_samples with weight 1 over the pixels (xs, ys), in numpy float32 (tests/resample_ref.py without its checks)."""
    c, n = conv[ys, xs], cnt[ys, xs, 0]
    with np.errstate(all="ignore"):
        capped = np.fmin(n, np.fmax(F(max_history) - F(1), F(0))) if max_history > 0 else n
        s = np.where(~np.isfinite(n) | (n < 0), F(0), capped).astype(F)
        a = F(1) / (s + F(1))
        ia = F(1) - a
        new = np.empty_like(c)
        new[:, :3] = t[:, :3] * a[:, None] + c[:, :3] * ia[:, None]
        new[:, 3] = a * a + c[:, 3] * ia
    conv[ys, xs] = new
    cnt[ys, xs] = 0
    cnt[ys, xs, 0] = s + F(1)


def run_size(ctx, dev, name, args, results):
    w, h = SIZES[name]
    m = RayTraceMaster(ctx, scenes.config3(w, h))
    m.EnableTemporalAccumulation()
    for _ in range(4):
        m.OnRenderImage()
    m.MoveCamera(*scenes.camera_matrices(w, h, position=(0.6, 1.0, -10.0), yaw_deg=3.0))
    mh = m._temporal["max_history"]
    conv, cnt = m._converged, m._tcount
    cnt_keep, spare = RenderTexture(ctx, w, h), RenderTexture(ctx, w, h)
    blit = lambda s, d: ctx.check(ctx.lib.urt_blit(ctx._h, s.handle, d.handle))  # noqa: E731
    blit(cnt, cnt_keep)
    m._bind_for_queries()                                           # the uniforms of the next frame, a Result texture
    m.InitRenderTexture()
    m.RayTraceShader.SetTexture(0, "Result", m._target)
    n = len(ctx.select_pixels(cnt, 1.0))
    share = n / (w * h)
    pixels = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    out = C.c_int()

    def select():
        ctx.check(ctx.lib.urt_select_pixels(ctx._h, cnt.handle, 1.0, C.c_void_p(pixels.data_ptr()), n, C.byref(out)))

    def select_count_only():
        ctx.check(ctx.lib.urt_select_pixels(ctx._h, cnt.handle, 1.0, None, 0, C.byref(out)))

    def restore():
        blit(cnt_keep, cnt)

    def resample():
        ctx.check(ctx.lib.urt_resample_below(ctx._h, conv.handle, cnt.handle, 1.0, m.numRays, m.numBounces, 1.0, mh, C.byref(out)))

    def pair():
        restore()
        resample()
        assert out.value == n, (out.value, n)

    forms = [("select", select), ("blit_same_size", lambda: blit(cnt_keep, spare)), ("select_count_only", select_count_only),
             ("resample_pair", pair), ("restore", restore)]
    ms = {k: [] for k, _ in forms}
    for _ in range(args.repeats):
        for k, fn in forms:
            ms[k].append(timed(fn, args.iters, args.warmup))
    info = {"width": w, "height": h, "selected": n, "selected_share": share, "samples": m.numRays, "bounces": m.numBounces}
    report(results, name, "select", ms["select"], **info, vs_blit=float(np.median(ms["select"]) / np.median(ms["blit_same_size"])))
    report(results, name, "blit_same_size", ms["blit_same_size"], **info)
    report(results, name, "select_count_only", ms["select_count_only"], **info)
    diff = [a - b for a, b in zip(ms["resample_pair"], ms["restore"])]
    report(results, name, "resample", diff, **info, ms_pair=[round(x, 4) for x in ms["resample_pair"]], ms_restore=[round(x, 4) for x in ms["restore"]])

    def wall(fn, before):
        t = []
        for _ in range(args.repeats):
            fn_total = 0.0
            for _ in range(args.wall_iters):
                before()
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                fn_total += time.perf_counter() - t0
            t.append(fn_total * 1e3 / args.wall_iters)
        return t

    def host_route():
        count = cnt.GetPixels()
        image = conv.GetPixels()
        ys, xs = np.nonzero(~(count[..., 0] >= 1.0))
        fresh = m.ResamplePixels(np.stack([xs, ys], axis=1).astype(np.int32))
        host_blend(image, count, ys, xs, fresh, mh)
        conv.SetPixels(image)
        cnt.SetPixels(count)

    restore(); resample(); ctx.synchronize()                        # both warm
    wall_gpu = wall(resample, restore)
    restore(); host_route()
    wall_host = wall(host_route, restore)
    report(results, name, "resample_wall", wall_gpu, **info)
    report(results, name, "host_route", wall_host, **info, vs_resample_wall=float(np.median(wall_host) / np.median(wall_gpu)))

    # the two routes give the same image and counts
    restore(); blit(conv, spare); resample()
    a = (conv.GetPixels(), cnt.GetPixels())
    restore(); blit(spare, conv); host_route()
    b = (conv.GetPixels(), cnt.GetPixels())
    r = {"size": name, "routes_agree_bitwise": bool(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes())}
    print(json.dumps(r), flush=True)
    results.append(r)
    for t in (cnt_keep, spare):
        t.Release()
    m.OnDisable()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,2160p")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--wall-iters", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    ctx = Context(0)
    stream = torch.cuda.Stream(dev)                                 # a real stream (torch's default one is handle 0 = "the library's own")
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)                              # the calls go where the events are recorded
    for name in args.sizes.split(","):
        run_size(ctx, dev, name, args, results)
    ctx.set_stream(None)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
