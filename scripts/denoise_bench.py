"""Time of the edge-aware a-trous denoiser (include/urt.h urt_denoise) per call, with and without albedo demodulation, at 1920x1080 and
3840x2160 and 1 and 5 iterations, on random guide images (tests/test_gpu_denoise.py random_inputs: ~10 % pass-through pixels).

Timing: device events on a torch stream the context is set to issue on, around `--iters` calls, after `--warmup` calls; each form is
measured in `--repeats` repeats and the median and spread are reported.  One JSON line per (size, iterations, albedo); --json writes them
all.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (the timed run has no profiler attached).
The bytes a pass must move at the least (25 taps x 32 B of colour and guide per pixel, from the caches; one 16-B store) are reported as
`tap_bytes_per_pass`, so that an effective cache bandwidth can be read off the kernel times.

    python scripts/denoise_bench.py [--sizes 1080p,2160p] [--iterations 1,5] [--iters 20] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context  # noqa: E402
from unityraytracer_amd.unity_api import RenderTexture  # noqa: E402

SIZES = {"1080p": (1920, 1080), "2160p": (3840, 2160)}


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


def main():
    from test_gpu_denoise import random_inputs
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,2160p")
    ap.add_argument("--iterations", default="1,5")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    ctx = Context(0)
    stream = torch.cuda.Stream(dev)                             # a real stream (torch's default one is handle 0 = "the library's own")
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)                          # the calls go where the events are recorded
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        color, hit, normal, albedo = random_inputs(1, w, h, bad_color=0.0)
        tex = [RenderTexture(ctx, w, h) for _ in range(5)]
        for t, a in zip(tex, (color, hit, normal, albedo)):
            t.SetPixels(a)
        src, ht, nt, at, dst = tex
        for it in (int(v) for v in args.iterations.split(",")):
            for with_albedo in (True, False):
                fn = lambda: ctx.denoise(src, dst, ht, nt, at if with_albedo else None, iterations=it)  # noqa: E731
                ms = [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)]
                r = {"size": name, "width": w, "height": h, "iterations": it, "albedo": with_albedo, "ms": ms,
                     "ms_median": float(np.median(ms)), "spread_pct": float((max(ms) - min(ms)) / np.median(ms) * 100),
                     "mpixels_s_median": float(w * h / (np.median(ms) * 1e3)), "tap_bytes_per_pass": w * h * (25 * 32 + 16)}
                print(json.dumps(r), flush=True)
                results.append(r)
        for t in tex:
            t.Release()
    ctx.set_stream(None)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
