"""Throughput of the batched ray queries (include/urt.h urt_ray_query_device) in Mrays/s, closest hit and any hit, on device-resident rays:

  C3 / C3D   camera rays at 1920x1080 from the scene's matrices (one per pixel centre, generated on the host)
  C5         4 M seeded random rays from points inside C5's bounds
  shadow     C5 surface points (closest hits of the random set, lifted 1e-3 along the normal) to a fixed light, t_max at the light

Timing: device events on a torch stream the context is set to issue on, around `--iters` queries, after `--warmup` queries; each set
is measured in `--repeats` repeats and the median and spread are reported.  One JSON line per (set, form); --json writes them all.

    python scripts/ray_query_bench.py [--sets C3,C3D,C5,shadow] [--iters 10] [--repeats 3] [--json out.json]
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


def camera_rays(sc, w=1920, h=1080):
    """RS:142-153 CreateCameraRay at every pixel centre (float64 on the host, then float32: a workload, not a parity check)."""
    c2w = np.asarray(sc.camera_to_world, np.float64).reshape(4, 4).T
    invp = np.asarray(sc.camera_inverse_projection, np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs + 0.5) / w * 2 - 1
    v = (ys + 0.5) / h * 2 - 1
    p = np.stack([u, v, np.zeros_like(u), np.ones_like(u)], -1).reshape(-1, 4) @ invp.T
    d = np.concatenate([p[:, :3], np.zeros((len(p), 1))], 1) @ c2w.T
    d = d[:, :3] / np.linalg.norm(d[:, :3], axis=1, keepdims=True)
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return o.astype(np.float32), d.astype(np.float32)


def bounds_rays(sc, n, seed):
    lo, hi = scenes.mesh_bounds(sc.mesh_objects, sc.vertices, sc.indices)
    lo, hi = lo.min(0), hi.max(0)
    rng = np.random.default_rng(seed)
    o = lo + rng.random((n, 3)) * (hi - lo)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def time_query(ctx, rays, out, n, flags, iters, warmup):
    lib, h = ctx.lib, ctx._h
    for _ in range(warmup):
        ctx.check(lib.urt_ray_query_device(h, rays.data_ptr(), n, out.data_ptr(), flags))
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        ctx.check(lib.urt_ray_query_device(h, rays.data_ptr(), n, out.data_ptr(), flags))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C3,C3D,C5,shadow")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--n-random", type=int, default=1 << 22)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    ctx = Context(0)
    stream = torch.cuda.Stream(dev)                             # a real stream (torch's default one is handle 0 = "the library's own")
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)                          # the queries go where the events are recorded
    wanted = args.sets.split(",")
    c5 = None
    for name in wanted:
        t0 = time.time()
        if name in ("C3", "C3D"):
            sc = scenes.CONFIGS[name]()
            O, D = camera_rays(sc)
            tm = np.full(len(O), np.inf, np.float32)
        else:
            if c5 is None:
                c5 = scenes.config5(64, 36)
            sc = c5
            O, D = bounds_rays(sc, args.n_random, 0x5EED)
            tm = np.full(len(O), np.inf, np.float32)
        m = RayTraceMaster(ctx, sc)
        m.Raycast((0, 1, 0), (0, 1, 0))                            # binds and prepares the scene
        if name == "shadow":
            hits = ctx.ray_query(O, D)
            sel = hits["kind"] == 3
            p = hits["position"][sel] + np.float32(1e-3) * hits["normal"][sel]
            light = np.array([0.0, 50.0, 0.0], np.float32)
            D = (light - p).astype(np.float32)
            tm = np.linalg.norm(D, axis=1).astype(np.float32)
            D = (D / tm[:, None]).astype(np.float32)
            O = p.astype(np.float32)
        n = len(O)
        rays = torch.from_numpy(np.concatenate([O, tm[:, None], D, np.zeros((n, 1), np.float32)], 1)).to(dev).contiguous()
        prep_s = time.time() - t0
        for flags, form in ((0, "closest"), (1, "any")):
            out = torch.empty(n * 12 if flags == 0 else n, dtype=torch.float32 if flags == 0 else torch.int32, device=dev)
            ms = [time_query(ctx, rays, out, n, flags, args.iters, args.warmup) for _ in range(args.repeats)]
            mr = [n / (t * 1e3) for t in ms]
            if flags == 1:
                frac = float(out.float().mean())
            else:
                frac = float((out.view(n, 12).view(torch.int32)[:, 7] != 0).float().mean())
            r = {"set": name, "form": form, "rays": n, "ms": ms, "mrays_s_median": float(np.median(mr)),
                 "spread_pct": float((max(mr) - min(mr)) / np.median(mr) * 100), "hit_fraction": frac, "setup_s": round(prep_s, 2)}
            print(json.dumps(r), flush=True)
            results.append(r)
        m.OnDisable()
    ctx.set_stream(None)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
