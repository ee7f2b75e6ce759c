"""Time of the depth of field (include/urt.h urt_depth_of_field, RayTraceMaster.EnableDepthOfField) at 1920x1080 on a rendered C3 frame,
for three depth fields:
  in_focus     every pixel at the focus distance (a = 0.5 everywhere: the tile reach is 0);
  c3           the hit target urt_render_aov writes for the C3 camera, focused at its median hit distance, Unity's physical-camera
               defaults (unity_api.dof_scale: 50 mm, f/5.6, a 24 mm sensor) and max_radius = 8;
  all_blurred  every pixel at +inf with scale = max_radius = 16 (the tile reach is 16 everywhere: 1089 taps a pixel).

Cases, per depth field.  Device calls are timed with events on a stream the context issues on, after `--warmup` calls, over `--iters`
calls, in `--repeats` repeats (median and spread reported), the cases alternating within every repeat:
  dof        urt_depth_of_field: k_dof_coc and k_dof_gather;
  dof_coc    the same call with URT_DOF_FLAG_COC: k_dof_coc alone (with its pointwise write of dst), so dof - dof_coc is about the gather;
  bloom      urt_bloom with the defaults, out of place, on the same image;
  blit       urt_blit of the same image;
  copy       a device-to-device copy of one RGBA32F image.
And, on the c3 depth field, with a host clock around `--iters` calls that end with one synchronisation:
  master_tonemap / master_dof_tonemap    RayTraceMaster.ToneMap() without and with EnableDepthOfField() (the guide is rendered per call).

`library` in every line names the library the run loaded (URT_LIB_PATH; "product" without it): the A/Bs in profiles/r27_logs/ ran this
script once per library, alternating in one session, the other libraries built from this tree with one of the patches there applied
(dof_fixed_reach.patch -> libdof_fixed, dof_lds48.patch -> libdof_lds48, dof_unpadded.patch -> libdof_unpadded).

    python scripts/dof_bench.py [--size 1920x1080] [--iters 200] [--repeats 5] [--json out.json]
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
from unityraytracer_amd.unity_api import RenderTexture, dof_scale  # noqa: E402

F = np.float32


def summary(ms):
    med = float(np.median(ms))
    return {"ms": [round(v, 5) for v in ms], "ms_median": round(med, 5), "spread_pct": round(float((max(ms) - min(ms)) / med * 100), 2) if med > 0 else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--iters", type=int, default=200)           # 200 calls of 0.01 .. 2 ms: 2 .. 400 ms a timed window
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

    W, H = (int(v) for v in args.size.split("x"))
    n = W * H
    ctx = Context(0)
    m = RayTraceMaster(ctx, scenes.config3(W, H))
    for _ in range(args.frames):
        m.OnRenderImage()
    ctx.synchronize()
    src = m._converged
    hit_c3 = m.RenderFeatureBuffers()[0]
    z = hit_c3.GetPixels()[..., 3]
    focus = float(np.median(z[np.isfinite(z)]))
    fields = {}
    for name, depth in (("in_focus", focus), ("all_blurred", np.inf)):
        t = RenderTexture(ctx, W, H)
        px = np.zeros((H, W, 4), F)
        px[..., 3] = depth
        t.SetPixels(px)
        fields[name] = t
    cases = {"in_focus": (fields["in_focus"], {"focus_distance": focus, "scale": 8.0, "max_radius": 8.0}),
             "c3": (hit_c3, {"focus_distance": focus, "scale": float(dof_scale(H, focus)), "max_radius": 8.0}),
             "all_blurred": (fields["all_blurred"], {"focus_distance": focus, "scale": 16.0, "max_radius": 16.0})}
    out = RenderTexture(ctx, W, H)
    a_img, b_img = torch.ones((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    # ---- device calls, events on the stream the context issues on ----
    stream = torch.cuda.Stream(dev)                             # a real stream (torch's default one is handle 0 = "the library's own")
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

    for name, (hit, params) in cases.items():
        def dof(flags):
            p = _lib.DofParams(params["focus_distance"], params["scale"], params["max_radius"], flags)
            return lambda: ctx.check(ctx.lib.urt_depth_of_field(ctx._h, src.handle, hit.handle, out.handle, C.byref(p)))

        calls = {
            "dof": dof(0),
            "dof_coc": dof(_lib.URT_DOF_FLAG_COC),
            "bloom": lambda: ctx.check(ctx.lib.urt_bloom(ctx._h, src.handle, out.handle, None, None)),
            "blit": lambda: ctx.check(ctx.lib.urt_blit(ctx._h, src.handle, out.handle)),
            "copy": lambda: b_img.copy_(a_img),
        }
        ms = {c: [] for c in calls}
        for _ in range(args.repeats):                           # alternate the cases within every repeat
            for c, fn in calls.items():
                ms[c].append(timed(fn, args.iters))
        for c in calls:
            r = {"width": W, "height": H, "depth": name, "case": c, **summary(ms[c]), **({k: round(v, 4) for k, v in params.items()} if c.startswith("dof") else {})}
            if c == "dof":
                r["gather_ms"] = round(r["ms_median"] - float(np.median(ms["dof_coc"])), 5)
            emit(r)
    ctx.set_stream(None)
    torch.cuda.set_stream(torch.cuda.default_stream(dev))

    # ---- RayTraceMaster.ToneMap(), host clock, one synchronisation at the end of every repeat ----
    def master_case(on):
        if on:
            m.EnableDepthOfField(**cases["c3"][1])
        else:
            m.DisableDepthOfField()
        for _ in range(args.warmup):
            m.ToneMap()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            m.ToneMap()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    steps = {"master_tonemap": False, "master_dof_tonemap": True}
    ms = {c: [] for c in steps}
    for _ in range(args.repeats):
        for c, on in steps.items():
            ms[c].append(master_case(on))
    for c in steps:
        r = {"width": W, "height": H, "depth": "c3", "case": c, **summary(ms[c])}
        if "dof" in c:
            r["dof_cost_ms"] = round(r["ms_median"] - float(np.median(ms["master_tonemap"])), 4)
        emit(r)
    for t in list(fields.values()) + [out]:
        t.Release()
    m.OnDisable()
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
