"""Time of the motion blur (include/urt.h urt_motion_blur, RayTraceMaster.EnableMotionBlur) at 1920x1080 and 3840x2160 on a rendered C3
frame, for three motion images:
  still   no pixel moves: every tile is a still tile and the gather is a copy — what every frame pays once the stage is on;
  pan     the whole image moves by (32, 0) with shutter = 1: every pixel gathers 33 taps, the full 16-pixel radius;
  c3      the motion image RayTraceMaster's reprojection writes after a MoveObjects of C3's first mesh (0.3 units along x), shutter = 1.

Cases, per motion image.  Device calls are timed with events on a stream the context issues on, after `--warmup` calls, over `--iters`
calls, in `--repeats` repeats (median and spread reported), the cases alternating within every repeat:
  blur       urt_motion_blur: k_mb_velocity and k_mb_gather;
  velocity   the same call with URT_MOTION_BLUR_FLAG_VELOCITY: k_mb_velocity and a gather that only writes (n.x, n.y, l_p, alpha), so
             blur - velocity is what the taps cost;
  copy       a device-to-device copy of one RGBA32F image: the yardstick.
Every line also gives the call's compulsory traffic (what the arithmetic of include/urt.h has to move once: src 16 B, motion .xyz 12 B,
hit.w 4 B, {l, z} 8 B written and read again, dst 16 B per pixel — 64 B for blur, 32 B for the copy) and the rate that is of the copy's.
`gather_fraction` is the part of the pixels that lie in tiles that are gathered (mn >= 0.25), read back from a VELOCITY call.

`library` in every line names the library the run loaded (URT_LIB_PATH; "product" without it), for A/Bs of builds in one session.

    python scripts/motion_blur_bench.py [--sizes 1920x1080,3840x2160] [--iters 200] [--repeats 5] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context, RayTraceMaster, _lib, scenes  # noqa: E402
from unityraytracer_amd.unity_api import RenderTexture  # noqa: E402

F = np.float32
BLUR_BYTES, COPY_BYTES = 64, 32                                 # compulsory traffic per pixel (see above)


def summary(ms):
    med = float(np.median(ms))
    return {"ms": [round(v, 5) for v in ms], "ms_median": round(med, 5), "spread_pct": round(float((max(ms) - min(ms)) / med * 100), 2) if med > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--iters", type=int, default=200)           # 200 calls of 0.05 .. 2 ms: 10 .. 400 ms a timed window
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    library = os.path.splitext(os.path.basename(os.environ["URT_LIB_PATH"]))[0] if os.environ.get("URT_LIB_PATH") else "product"
    results = []

    def emit(r):
        r = {"library": library, **r}
        print(json.dumps(r), flush=True)
        results.append(r)

    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        n = W * H
        ctx = Context(0)
        sc = scenes.config3(W, H)
        m = RayTraceMaster(ctx, sc)
        m.EnableTemporalAccumulation()
        m.EnableMotionBlur(shutter=1.0)
        for _ in range(args.frames):
            m.OnRenderImage()
        moved = np.array(sc.mesh_objects[0]["localToWorldMatrix"], F).reshape(16).copy()
        moved[12] += F(0.3)                                     # Unity memory order: the translation is entries 12..14
        m.MoveObjects({0: moved})
        m.OnRenderImage()
        m.ToneMap()                                             # renders the hit guide (m._dofHit) the blur uses
        ctx.synchronize()
        src, hit = m._converged, m._dofHit
        motions = {"c3": m._mbMotion}
        for name, mx in (("still", 0.0), ("pan", 32.0)):
            t = RenderTexture(ctx, W, H)
            px = np.zeros((H, W, 4), F)
            px[..., 0], px[..., 2] = mx, 1.0
            t.SetPixels(px)
            motions[name] = t
        out = RenderTexture(ctx, W, H)
        a_img, b_img = torch.ones((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

        stream = torch.cuda.Stream(dev)                         # a real stream (torch's default one is handle 0 = "the library's own")
        torch.cuda.set_stream(stream)
        ctx.set_stream(stream.cuda_stream)

        def timed(call, iters):
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                call()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / iters

        for name in ("still", "pan", "c3"):
            motion = motions[name]

            def blur(flags):
                p = _lib.MotionBlurParams(1.0, 16.0, flags, 0)
                return lambda: ctx.check(ctx.lib.urt_motion_blur(ctx._h, src.handle, motion.handle, hit.handle, out.handle, C.byref(p)))

            blur(_lib.URT_MOTION_BLUR_FLAG_VELOCITY)()
            v = out.GetPixels()
            gathered = float(((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) >= 0.25).mean())
            calls = {"blur": blur(0), "velocity": blur(_lib.URT_MOTION_BLUR_FLAG_VELOCITY), "copy": lambda: b_img.copy_(a_img)}
            ms = {c: [] for c in calls}
            for _ in range(args.repeats):                       # alternate the cases within every repeat
                for c, fn in calls.items():
                    ms[c].append(timed(fn, args.iters))
            copy_rate = COPY_BYTES * n / float(np.median(ms["copy"]))
            for c in calls:
                r = {"width": W, "height": H, "motion": name, "case": c, **summary(ms[c])}
                if c == "blur":
                    r["gather_fraction"] = round(gathered, 4)
                    r["taps_ms"] = round(r["ms_median"] - float(np.median(ms["velocity"])), 5)
                    r["compulsory_bytes_per_pixel"] = BLUR_BYTES
                    r["of_copy_rate"] = round(BLUR_BYTES * n / r["ms_median"] / copy_rate, 3)
                    r["copies"] = round(r["ms_median"] / float(np.median(ms["copy"])), 2)
                emit(r)
        ctx.set_stream(None)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        for t in (motions["still"], motions["pan"], out):
            t.Release()
        m.OnDisable()
        ctx.close()
        del a_img, b_img
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
