"""Time of "trace at low resolution, present at full" (include/urt.h urt_upsample, RayTraceMaster.Upscale) against a full-size frame, on
C3 (1920x1080 presented) and C4 (3840x2160 presented), the radiance traced on a grid 2 and 3 times smaller along each axis.

Cases, per configuration and divisor.  A step is what a host that moves the camera every frame pays per presented image; it is timed with
a host clock around `--iters` steps that end in a device synchronise, after `--warmup` steps, in `--repeats` repeats (median and spread
reported), the cases alternating within every repeat:
  full_frame    (a) one full-size frame: OnRenderImage and a flush — the library without this feature;
  low_upsample  (b) one low-grid frame, the feature buffers on both grids (urt_render_aov twice) and urt_upsample: OnRenderImage + Upscale;
  low_fill      (c) (b) with fill_holes: the pixels no low-resolution tap serves are traced at full resolution (`filled` = their number);
  upsample      (d) urt_upsample alone (device events on a stream the context issues on), as GB/s of its compulsory traffic — per full-grid
                pixel 48 B of feature texels in and 32 B of colour and count out, per low-grid texel 80 B read once — beside the
                device-to-device copy rate measured here as scripts/skin_bench.py measures it (urt_buffer_set_data_device, 32 M
                elements of 12 B, bytes read + written).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python scripts/upsample_bench.py [--configs C3,C4] [--divisors 2,3] [--iters 20] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context, RayTraceMaster, scenes  # noqa: E402
from unityraytracer_amd.unity_api import ComputeBuffer, RenderTexture  # noqa: E402

CONFIGS = {"C3": (scenes.config3, 1920, 1080), "C4": (scenes.config4, 3840, 2160)}


def summary(ms):
    med = float(np.median(ms))
    return {"ms": [round(v, 4) for v in ms], "ms_median": round(med, 4), "spread_pct": round(float((max(ms) - min(ms)) / med * 100), 2) if med > 0 else 0.0}


def copy_rate(ctx):
    """The device-to-device copy rate of scripts/skin_bench.py: urt_buffer_set_data_device on 32 M elements of 12 bytes."""
    big_n, reps = 32 << 20, 30
    big = ComputeBuffer(ctx, big_n, 12)
    src = torch.ones((big_n, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fn = lambda: ctx.check(ctx.lib.urt_buffer_set_data_device(ctx._h, big.handle, 0, src.data_ptr(), big_n))  # noqa: E731
    fn(); ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    big.Release()
    return ms, 2 * 12 * big_n / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C4")
    ap.add_argument("--divisors", default="2,3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    ctx = Context(0)
    copy_ms, copy_gbs = copy_rate(ctx)
    r = {"case": "copy", "elements": 32 << 20, "ms": round(copy_ms, 4), "GBps": round(copy_gbs, 1)}
    print(json.dumps(r), flush=True)
    results.append(r)

    def host_timed(c, step):
        for _ in range(args.warmup):
            step()
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            step()
        c.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    for name in args.configs.split(","):
        make, W, H = CONFIGS[name]
        full = RayTraceMaster(ctx, make(W, H))
        full.OnRenderImage()
        ctx.synchronize()

        def full_step():
            full.OnRenderImage()
            ctx.flush()

        low_ctx = Context(0)                                    # a context of its own: alternating the cases re-prepares no scene

        for d in (int(v) for v in args.divisors.split(",")):
            w, h = W // d, H // d
            m = RayTraceMaster(low_ctx, make(w, h))
            m.OnRenderImage()
            filled = []

            def up_step():
                m.OnRenderImage()
                m.Upscale(W, H)

            def fill_step():
                m.OnRenderImage()
                m.Upscale(W, H, fill_holes=True)
                filled.append(m.upscaleFilled)

            cases = {"full_frame": (ctx, full_step), "low_upsample": (low_ctx, up_step), "low_fill": (low_ctx, fill_step)}
            ms = {c: [] for c in cases}
            for _ in range(args.repeats):                       # alternate the cases within every repeat
                for c, (on, fn) in cases.items():
                    ms[c].append(host_timed(on, fn))
            for c in cases:
                r = {"config": name, "divisor": d, "case": c, "width": W, "height": H, "low_width": w, "low_height": h, **summary(ms[c])}
                if c == "low_fill":
                    r["filled_median"] = int(np.median(filled))
                    r["filled_share"] = round(float(np.median(filled)) / (W * H), 5)
                if c != "full_frame":
                    r["of_full_frame"] = round(r["ms_median"] / float(np.median(ms["full_frame"])), 3)
                print(json.dumps(r), flush=True)
                results.append(r)

            # (d) the kernel's call alone, on the textures the master has just filled
            m.Upscale(W, H)
            low_ctx.synchronize()
            holes = float((m._upcount.GetPixels()[..., 0] == 0).mean())
            stream = torch.cuda.Stream(dev)                     # a real stream (torch's default one is handle 0 = "the library's own")
            torch.cuda.set_stream(stream)
            low_ctx.set_stream(stream.cuda_stream)              # the calls go where the events are recorded
            low_hit, low_normal, _, low_id = m._uplow
            hit, normal, albedo, ids = m._upaov
            out, cnt = RenderTexture(low_ctx, W, H), RenderTexture(low_ctx, W, H)

            def call():
                low_ctx.upsample(m._converged, low_hit, low_normal, low_id, hit, normal, ids, out, cnt, albedo=albedo, sky_from_albedo=True)

            ev = []
            for _ in range(args.repeats):
                for _ in range(args.warmup):
                    call()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters * 5):
                    call()
                b.record()
                b.synchronize()
                ev.append(a.elapsed_time(b) / (args.iters * 5))
            low_ctx.set_stream(None)
            torch.cuda.set_stream(torch.cuda.default_stream(dev))
            nbytes = W * H * 80 + w * h * 80
            s = summary(ev)
            gbs = nbytes / (s["ms_median"] * 1e-3) / 1e9
            r = {"config": name, "divisor": d, "case": "upsample", "width": W, "height": H, "low_width": w, "low_height": h, **s,
                 "bytes": nbytes, "GBps": round(gbs, 1), "of_copy": round(gbs / copy_gbs, 3), "holes_share": round(holes, 5)}
            print(json.dumps(r), flush=True)
            results.append(r)
            out.Release(); cnt.Release()
            m.OnDisable()
        low_ctx.close()
        full.OnDisable()
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
