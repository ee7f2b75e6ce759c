"""Time of the per-pixel first-hit feature buffers (include/urt.h urt_render_aov) per call and in Mpixels/s, with all four targets and
with `hit` only, and of urt_ray_query_device on the same pixel-centre rays (camera rays built on the host with the same arithmetic,
bit-identical results: tests/test_gpu_aov.py), so that the tiled camera-ray kernel and the row-fed query are compared on one workload.

  C3 / C3D   1920x1080        C4 / C5   3840x2160

Timing: device events on a torch stream the context is set to issue on, around `--iters` calls, after `--warmup` calls; each form is
measured in `--repeats` repeats and the median and spread are reported.  One JSON line per (set, form); --json writes them all.  Kernel
times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (the timed run has no profiler attached).

    python scripts/aov_bench.py [--sets C3,C3D,C4,C5] [--iters 10] [--repeats 3] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context, RayTraceMaster, scenes  # noqa: E402
from unityraytracer_amd.unity_api import RenderTexture  # noqa: E402

SIZES = {"C3": (1920, 1080), "C3D": (1920, 1080), "C4": (3840, 2160), "C5": (3840, 2160)}


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
    from test_gpu_aov import camera_rays                        # the normative float32 camera rays (the AOV kernel's own)
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C3,C3D,C4,C5")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    ctx = Context(0)
    stream = torch.cuda.Stream(dev)                             # a real stream (torch's default one is handle 0 = "the library's own")
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)                          # the calls go where the events are recorded
    for name in args.sets.split(","):
        t0 = time.time()
        w, h = SIZES[name]
        sc = scenes.CONFIGS[name]()
        m = RayTraceMaster(ctx, sc)
        m.screen_width, m.screen_height = w, h
        m.Raycast((0, 1, 0), (0, 1, 0))                            # binds and prepares the scene
        tex = [RenderTexture(ctx, w, h) for _ in range(4)]
        O, D = camera_rays(sc, w, h)
        n = w * h
        rays = torch.from_numpy(np.concatenate([O.reshape(n, 3), np.full((n, 1), np.inf, np.float32), D.reshape(n, 3),
                                                np.zeros((n, 1), np.float32)], 1)).to(dev).contiguous()
        out = torch.empty(n * 12, dtype=torch.float32, device=dev)
        setup_s = time.time() - t0
        forms = (("aov_all", lambda: ctx.render_aov(*tex)),
                 ("aov_hit", lambda: ctx.render_aov(hit=tex[0])),
                 ("query_closest", lambda: ctx.check(ctx.lib.urt_ray_query_device(ctx._h, rays.data_ptr(), n, out.data_ptr(), 0))))
        for form, fn in forms:
            ms = [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)]
            mp = [n / (t * 1e3) for t in ms]
            r = {"set": name, "form": form, "width": w, "height": h, "ms": ms, "ms_median": float(np.median(ms)),
                 "mpixels_s_median": float(np.median(mp)), "spread_pct": float((max(mp) - min(mp)) / np.median(mp) * 100),
                 "setup_s": round(setup_s, 2)}
            print(json.dumps(r), flush=True)
            results.append(r)
        torch.cuda.synchronize()
        q = out.view(n, 12)
        same = bool(torch.equal(q[:, 0].view(h, w), torch.from_numpy(tex[0].GetPixels()[..., 3]).to(dev)))
        print(json.dumps({"set": name, "aov_distance_equals_query": same}), flush=True)
        results.append({"set": name, "aov_distance_equals_query": same})
        for t in tex:
            t.Release()
        m.OnDisable()
    ctx.set_stream(None)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
