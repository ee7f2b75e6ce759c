"""Time of the temporal reprojection (include/urt.h urt_reproject) and of the history blend (urt_blit_add_history) at 1920x1080 and
3840x2160, on the analytic feature buffers of tests/reproject_ref.py (a small camera move: most pixels keep their history).

Cases, each timed with device events on a torch stream the context is set to issue on, `--iters` calls after `--warmup`, in `--repeats`
repeats (median and spread reported):
  reproject        one urt_reproject call with a motion image;
  blend            one urt_blit_add_history call that is not deferred (its source is not a pending frame);
  fused20_present  20 frames of C1 (16 spheres, 1 bounce), each dispatched, blended with urt_blit_add_history and presented, submitted
                   as one batch (frames_per_launch 20): the per-launch time minus that of the same 20 dispatches without the blends and
                   presents, i.e. the one fused pass, per launch.
With --motion, instead of the blend cases (urt_reproject_objects, per-object motion tables), `reproject` and these alternate in every
repeat, so that the three are compared under the same conditions:
  objects_static   urt_reproject_objects with tables that hold only identity entries (a static scene that still passes its tables);
  objects_moved    the same with every wall ("mesh") entry a small rigid motion: every mesh pixel loads its entry and takes the moved path
                   (`moved_share` is the share of such pixels in the image).
With --deform (urt_reproject_deformed, per-vertex motion) the two walls of the analytic scene become meshes: each is cut into a grid of
triangles of about six pixels at 1080p, every wall pixel's id texel names its triangle's index slot and barycentrics, and the previous
positions are the grid's vertices moved a little in the wall's plane.  `reproject`, `objects_moved` (as with --motion) and these alternate:
  deformed_static  urt_reproject_deformed with every flag zero (a scene that passes its buffers while nothing deforms);
  deformed_walls   both walls flagged: every mesh pixel gathers three indices, three vertices and its object's matrix
                   (`moved_share` is the share of such pixels in the image; --camera-z -1 brings it from 1.4 % to 11 %).
Bytes per pixel are the compulsory traffic (reproject: 48 B of current AOVs, 80 B of previous history and AOVs, 48 B out; blend: 64 B;
fused n frames with a present: 16 n + 64 B) and `of_6p3TBs` the fraction of the ~6.3 TB/s a float4 copy reaches on the chip.  Kernel times
come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python scripts/reproject_bench.py [--sizes 1080p,2160p] [--iters 20] [--repeats 5] [--motion | --deform] [--json out.json]
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

from unityraytracer_amd import Context, RayTraceMaster, scenes  # noqa: E402
from unityraytracer_amd.unity_api import ComputeBuffer, ComputeShader, RenderTexture  # noqa: E402

SIZES = {"1080p": (1920, 1080), "2160p": (3840, 2160)}
PEAK = 6.3e12


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


def report(name, case, w, h, ms, bpp, results):
    med = float(np.median(ms))
    r = {"size": name, "case": case, "width": w, "height": h, "ms": ms, "ms_median": med,
         "spread_pct": float((max(ms) - min(ms)) / med * 100) if med > 0 else 0.0, "bytes_per_pixel": bpp,
         "of_6p3TBs": float(w * h * bpp / (med * 1e-3) / PEAK) if med > 0 else 0.0}
    print(json.dumps(r), flush=True)
    results.append(r)


WALLS = {4: (6.0, (-4.0, 4.0), (0.0, 3.0), (128, 48)), 5: (2.0, (2.5, 4.5), (0.0, 1.6), (48, 40))}   # tests/reproject_ref.py default_objects; grid cells


def wall_meshes(hit, normal, ids, rng):
    """The two walls as triangle grids: (prev_vertices, indices) and, written into `ids`, every wall pixel's index slot and barycentrics.
    Cell (i, j) holds the triangles (c00, c01, c10) and (c11, c10, c01), wound so that their face normals look along -z as the walls do."""
    verts, index, first_slot = [], [], 0
    iv = ids.view(np.int32)
    for o, (zc, (x0, x1), (y0, y1), (gx, gy)) in WALLS.items():
        base = sum(len(v) for v in verts)
        X, Y = np.meshgrid(np.linspace(x0, x1, gx + 1), np.linspace(y0, y1, gy + 1))
        verts.append(np.stack([X, Y, np.full_like(X, zc)], -1).reshape(-1, 3))
        vid = lambda i, j: base + j * (gx + 1) + i  # noqa: E731
        I, J = np.meshgrid(np.arange(gx), np.arange(gy))
        tris = np.stack([np.stack([vid(I, J), vid(I, J + 1), vid(I + 1, J)], -1), np.stack([vid(I + 1, J + 1), vid(I + 1, J), vid(I, J + 1)], -1)], 2)
        index.append(tris.reshape(-1, 3))
        on = (normal[..., 3] == 3) & (iv[..., 0] == o)
        fx = np.clip((hit[..., 0].astype(np.float64) - x0) / (x1 - x0) * gx, 0, gx - 1e-9)
        fy = np.clip((hit[..., 1].astype(np.float64) - y0) / (y1 - y0) * gy, 0, gy - 1e-9)
        i, j = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        a, b = fx - i, fy - j
        upper = a + b > 1
        slot = first_slot + 3 * (2 * (j * gx + i) + upper)
        iv[..., 1] = np.where(on, slot, iv[..., 1])
        ids[..., 2] = np.where(on, np.where(upper, 1 - b, b), ids[..., 2]).astype(np.float32)
        ids[..., 3] = np.where(on, np.where(upper, 1 - a, a), ids[..., 3]).astype(np.float32)
        first_slot += 3 * 2 * gx * gy
    pv = np.concatenate(verts)
    pv[:, :2] += rng.uniform(-0.02, 0.02, (len(pv), 2))                       # where the vertices were: a little off, in the plane
    return pv.astype(np.float32), np.concatenate(index).astype(np.int32).reshape(-1)


def main():
    from reproject_ref import analytic_aovs
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,2160p")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--motion", action="store_true", help="time urt_reproject_objects (static and all-moved tables) next to urt_reproject")
    ap.add_argument("--deform", action="store_true", help="time urt_reproject_deformed (no mesh flagged, both walls flagged) next to urt_reproject and urt_reproject_objects")
    ap.add_argument("--camera-z", type=float, default=-10.0, help="z of both cameras (the walls stand at z = 2 and z = 6: nearer cameras see more mesh pixels)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    ctx = Context(0)
    stream = torch.cuda.Stream(dev)                             # a real stream (torch's default one is handle 0 = "the library's own")
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)                          # the calls go where the events are recorded
    rng = np.random.default_rng(1)
    for name in args.sizes.split(","):
        w, h = SIZES[name]
        cam_a = scenes.camera_matrices(w, h, position=(0.0, 1.0, args.camera_z))
        cam_b = scenes.camera_matrices(w, h, position=(0.1, 1.0, args.camera_z), yaw_deg=1.0)
        prev, cur = analytic_aovs(w, h, *cam_a), analytic_aovs(w, h, *cam_b)
        if args.deform:
            cur = [a.copy() for a in cur]
            prev_vertices, wall_indices = wall_meshes(*cur, rng)
        color = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
        count = np.zeros((h, w, 4), np.float32)
        count[..., 0] = 16.0
        tex = [RenderTexture(ctx, w, h) for _ in range(11)]
        for t, a in zip(tex, [color, count] + list(prev) + list(cur)):
            t.SetPixels(a)
        sh = ComputeShader(ctx)
        sh.SetMatrix("_CameraToWorld", cam_b[0])
        sh.SetMatrix("_CameraInverseProjection", cam_b[1])
        M = scenes.world_to_clip(*cam_a)
        if args.motion or args.deform:
            n = 6                                               # the analytic scene's ids: ground 0, spheres 1..3, walls ("meshes") 4 and 5
            ident = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (n, 1))
            moved = ident.copy()
            a = np.radians(2.0)
            moved[:, [0, 2, 6, 8]] = (np.cos(a), -np.sin(a), np.sin(a), np.cos(a))        # 2 degrees about y ...
            moved[:, 9:] = (0.05, 0.0, 0.02)                                              # ... and a small step
            bufs = {}
            for key, t in (("ident", ident), ("moved", moved)):
                bufs[key] = ComputeBuffer(ctx, n, 48)
                bufs[key].SetData(t)
            share = float((cur[1][..., 3] == 3).mean())
            cases = {"reproject": lambda: ctx.reproject(*tex[:10], M, motion=tex[10]),
                     "objects_static": lambda: ctx.reproject(*tex[:10], M, motion=tex[10], mesh_motion=bufs["ident"], sphere_motion=bufs["ident"]),
                     "objects_moved": lambda: ctx.reproject(*tex[:10], M, motion=tex[10], mesh_motion=bufs["moved"], sphere_motion=bufs["ident"])}
            if args.deform:
                objects = np.zeros((n, 28), np.float32)
                objects[:, [0, 5, 10, 15]] = 1.0                   # identity matrices: the walls' vertices are world positions
                flagged = np.zeros(n, np.int32)
                flagged[list(WALLS)] = 1
                for key, a, stride in (("pv", prev_vertices, 12), ("ix", wall_indices, 4), ("mo", objects, 112), ("none", np.zeros(n, np.int32), 4),
                                       ("walls", flagged, 4)):
                    bufs[key] = ComputeBuffer(ctx, a.nbytes // stride, stride)
                    bufs[key].SetData(a)
                del cases["objects_static"]
                for c, flags in (("deformed_static", "none"), ("deformed_walls", "walls")):
                    cases[c] = lambda flags=flags: ctx.reproject(*tex[:10], M, motion=tex[10], mesh_motion=bufs["ident"], sphere_motion=bufs["ident"],
                                                                 deform=(bufs["pv"], bufs["ix"], bufs["mo"], bufs[flags]))
            ms = {c: [] for c in cases}
            for _ in range(args.repeats):                       # alternate the cases within every repeat
                for c, fn in cases.items():
                    ms[c].append(timed(fn, args.iters, args.warmup))
            for c in cases:
                report(name, c, w, h, ms[c], 176, results)
                results[-1]["moved_share"] = share if c in ("objects_moved", "deformed_walls") else 0.0
            if args.deform:                                     # what the flagged walls keep: the cases must not time dead pixels
                ctx.reproject(*tex[:10], M, motion=tex[10], deform=(bufs["pv"], bufs["ix"], bufs["mo"], bufs["walls"]))
                kept = tex[9].GetPixels()[..., 0][cur[1][..., 3] == 3] > 0
                print(json.dumps({"size": name, "case": "deformed_walls_kept_share", "value": float(kept.mean()), "moved_share": share}), flush=True)
            for t in tex + list(bufs.values()):
                t.Release()
            continue
        fn = lambda: ctx.reproject(*tex[:10], M, motion=tex[10])  # noqa: E731
        report(name, "reproject", w, h, [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)], 176, results)
        fn = lambda: ctx.blit_add_history(tex[0], tex[8], tex[9], 64.0)  # noqa: E731
        report(name, "blend", w, h, [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)], 64, results)
        for t in tex:
            t.Release()

        # 20 deferred frames per launch, with and without the blends and presents
        ctx.set_stream(None)                                    # batching needs the library's own stream
        ctx.set_option("frames_per_launch", 20)
        sc = scenes.config1(w, h)
        m = RayTraceMaster(ctx, sc)
        m.EnableTemporalAccumulation()
        present = RenderTexture(ctx, w, h)
        m.OnRenderImage(present)
        ctx.synchronize()

        def batch(blend):
            def run():
                for _ in range(20):
                    if blend:
                        m.OnRenderImage(present)
                    else:
                        m.SetShaderParameters()
                        m.RayTraceShader.SetTexture(0, "Result", m._target)
                        m.RayTraceShader.Dispatch(0, (w + 7) // 8, (h + 7) // 8, 1)
                        m._frame += 1
                ctx.flush()
            return run

        def host_timed(fn):
            import time
            fn()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters // 4 or 1):
                fn()
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (args.iters // 4 or 1)

        with_b = [host_timed(batch(True)) for _ in range(args.repeats)]
        without = [host_timed(batch(False)) for _ in range(args.repeats)]
        diff = [a - b for a, b in zip(sorted(with_b), sorted(without))]
        r = {"size": name, "case": "fused20_batch", "ms_with_blends": with_b, "ms_without": without,
             "ms_with_median": float(np.median(with_b)), "ms_without_median": float(np.median(without))}
        print(json.dumps(r), flush=True)
        results.append(r)
        report(name, "fused20_present", w, h, diff, 16 * 20 + 64, results)
        present.Release()
        m.OnDisable()
        ctx.set_option("frames_per_launch", 0)
        ctx.set_stream(stream.cuda_stream)
    ctx.set_stream(None)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
