"""Cost of the normals of a mesh whose positions were written on the GPU, from the first call of an update to the finished in-place
update of the scene, two ways — every update puts another deformation of the rest positions into _Vertices with
ComputeBuffer.SetDataDevice from a torch tensor, then:
  (a) the host route: GetData of the deformed spans (a synchronising download), urt_host_compute_normals over the scene's lists, SetData
      of the normals of those spans, SetData of _MeshBVH, the preparation;
  (b) the device route: urt_compute_normals over plans made once (`plan_ms`), SetData of _MeshBVH, the preparation.
Cases: C3's blob (one MeshObject, 34,802 vertices, 1920x1080), C5 with one and with all twelve MeshObjects deformed.  `equal` says that
the normals (b) left in the buffer are those of (a), bit for bit (a NaN equal to a NaN); `downloads` counts device-to-host copies of
_Vertices / _Normals during (b).  Part `rate`: urt_compute_normals on a grid mesh of 16.8 M vertices / 33.5 M triangles — the face image
alone is 537 MB, twice the chip's 256 MB last-level cache, so the second kernel cannot find it there — as compulsory bytes per second,
every array read or written once, beside the device-to-device copy rate measured with urt_buffer_set_data_device on 32 M elements.
Part `kernels`: the same launches in a child process under `rocprofv3 --kernel-trace --stats` (the timed runs have no profiler
attached), which times k_face_normals and k_vertex_normals apart; it runs first, before this process uses the GPU.

    python scripts/normals_bench.py [--part kernels,update,rate] [--repeats 5] [--json out.json]
"""
import argparse
import copy
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process, tests/conftest.py)

from skin_bench import finish, spans, summary  # noqa: E402
from unityraytracer_amd import ComputeBuffer, Context, RayTraceMaster, host_scene, scenes  # noqa: E402

F = np.float32


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def deform(P, step):
    """A function of the rest position alone (coincident vertices stay coincident)."""
    return (P + F(0.02) * np.sin(F(3.0) * P[:, [1, 2, 0]] + F(0.37 * step))).astype(F)


def part_update(args, results):
    for cfg, size, which in (("C3", (1920, 1080), "one"), ("C5", (640, 360), "one"), ("C5", (640, 360), "all")):
        sc = scenes.CONFIGS[cfg](*size)
        n = len(sc.mesh_objects)
        meshes = [n - 1] if which == "one" else list(range(n))
        sp = spans(sc)
        lo, hi = min(sp[k][0] for k in meshes), max(sp[k][1] for k in meshes)
        poses = []
        for s in range(args.repeats + 1):
            v = sc.vertices.copy()
            for k in meshes:
                v[sp[k][0]: sp[k][1]] = deform(sc.vertices[sp[k][0]: sp[k][1]], s + 1)
            poses.append(v)
        heaps = [scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices)) for v in poses]
        dev = [torch.from_numpy(v[lo:hi]).cuda() for v in poses]
        torch.cuda.synchronize()
        base = {"part": "update", "config": cfg, "triangles": sc.n_triangles, "meshes": n, "deformed_per_update": len(meshes),
                "deformed_vertices": int(sum(sp[k][1] - sp[k][0] for k in meshes))}
        with Context(0) as ctx:
            m = RayTraceMaster(ctx, copy.copy(sc))
            m.OnRenderImage()
            ctx.synchronize()
            # (a) the host route that exists without urt_compute_normals
            host_v = sc.vertices.copy()
            t, normals_ms = [], []
            for tv, h in zip(dev, heaps):
                ctx.synchronize()
                t0 = time.perf_counter()
                m._vertexBuffer.SetDataDevice(tv, lo)
                for k in meshes:
                    a, b = sp[k]
                    host_v[a:b] = m._vertexBuffer.GetData(a, b - a).view(F).reshape(-1, 3)
                t1 = time.perf_counter()
                nr = host_scene.compute_normals(host_v, sc.indices)
                normals_ms.append((time.perf_counter() - t1) * 1e3)
                for k in meshes:
                    a, b = sp[k]
                    m._normalBuffer.SetData(nr, a, a, b - a)
                m._meshObjectBVHBuffer.SetData(h)
                finish(ctx)
                t.append((time.perf_counter() - t0) * 1e3)
            r = dict(base, path="a_get_data_host_normals_set_data")
            r.update(summary("update_ms", t[1:]))                                  # the first one warms up
            r.update(summary("host_normals_ms", normals_ms[1:]))
            r["downloads"] = ctx.buffer_state(m._vertexBuffer)["downloads"]
            print(json.dumps(r), flush=True); results.append(r)
            want = nr
            # (b) urt_compute_normals, ending on the pose (a) ended on.  The plans are made from a DEFORMED pose: C5's twelve meshes are one
            # icosphere in object space, so at rest every vertex welds with its eleven twins, and a mesh that is deformed alone leaves them
            m._vertexBuffer.SetData(poses[0]); m._normalBuffer.SetData(sc.normals); finish(ctx)
            t0 = time.perf_counter()
            plans = [ctx.normals_plan(m._vertexBuffer, m._indexBuffer, sp[k][0], sp[k][1] - sp[k][0]) for k in meshes]
            plan_ms = (time.perf_counter() - t0) * 1e3
            d0 = ctx.buffer_state(m._vertexBuffer)["downloads"] + ctx.buffer_state(m._normalBuffer)["downloads"]
            in_place0 = ctx.deform_stats()["renormed"]
            t = []
            for tv, h in zip(dev, heaps):
                ctx.synchronize()
                t0 = time.perf_counter()
                m._vertexBuffer.SetDataDevice(tv, lo)
                for p in plans:
                    p.compute(m._normalBuffer)
                m._meshObjectBVHBuffer.SetData(h)
                finish(ctx)
                t.append((time.perf_counter() - t0) * 1e3)
            r = dict(base, path="b_compute_normals")
            r.update(summary("update_ms", t[1:]))
            r["plan_ms"] = round(plan_ms, 3)
            r["max_valence"] = max(p.info["max_valence"] for p in plans)
            r["plan_device_bytes"] = sum(p.info["device_bytes"] for p in plans)
            r["downloads"] = ctx.buffer_state(m._vertexBuffer)["downloads"] + ctx.buffer_state(m._normalBuffer)["downloads"] - d0
            r["renormed_in_place"] = ctx.deform_stats()["renormed"] - in_place0
            got = m._normalBuffer.GetData().view(F).reshape(-1, 3)                 # (after the downloads were counted)
            r["equal"] = all(same(got[sp[k][0]: sp[k][1]], want[sp[k][0]: sp[k][1]]) for k in meshes)
            print(json.dumps(r), flush=True); results.append(r)
            for p in plans:
                p.Release()
            m.OnDisable()


def rate_bytes(nv, nt, ne):
    """Compulsory bytes of the two kernels: triangles and vertices read once and faces written; ranges, entries and faces read once and
    normals written."""
    return 12 * nt + 12 * nv + 16 * nt, 8 * nv + 4 * ne + 16 * nt + 12 * nv


def part_kernels(args, results):
    """The launches of part `rate` in a child under the profiler; the kernels' average durations from its kernel statistics."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--part", "rate"]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
        rate = [json.loads(line) for line in out.splitlines() if line.startswith("{")][-1]
        rows = [row for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True) for row in csv.DictReader(open(f))]
    r = {"part": "kernels", "vertices": rate["vertices"], "triangles": rate["triangles"], "entries": rate["entries"],
         "copy_GBps_in_the_child": rate["copy_GBps"]}
    for name, nbytes in zip(("k_face_normals", "k_vertex_normals"), rate_bytes(rate["vertices"], rate["triangles"], rate["entries"])):
        row = [x for x in rows if name in x["Name"]][0]
        ns = float(row["AverageNs"])
        r.update({name + "_calls": int(row["Calls"]), name + "_ms": round(ns * 1e-6, 4), name + "_bytes": nbytes,
                  name + "_GBps": round(nbytes / ns, 1), name + "_of_copy": round(nbytes / ns / rate["copy_GBps"], 3)})
    print(json.dumps(r), flush=True); results.append(r)


def part_rate(args, results):
    side, big_n, reps = 4096, 32 << 20, 20
    gx, gz = np.meshgrid(np.arange(side, dtype=F), np.arange(side, dtype=F), indexing="ij")
    v = np.stack([gx, np.sin(gx * F(0.05)) * np.cos(gz * F(0.07)), gz], axis=-1).reshape(-1, 3).astype(F)
    i = (np.arange(side - 1, dtype=np.int32)[:, None] * side + np.arange(side - 1, dtype=np.int32)[None, :]).reshape(-1)
    t = np.stack([i, i + 1, i + side, i + 1, i + side + 1, i + side], axis=1).reshape(-1).astype(np.int32)
    with Context(0) as ctx:
        V, I, D = ComputeBuffer(ctx, len(v), 12), ComputeBuffer(ctx, len(t), 4), ComputeBuffer(ctx, len(v), 12)
        V.SetData(v); I.SetData(t)
        t0 = time.perf_counter()
        plan = ctx.normals_plan(V, I)
        plan_ms = (time.perf_counter() - t0) * 1e3
        info = plan.info
        big = ComputeBuffer(ctx, big_n, 12)
        src = torch.ones((big_n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def timed(fn, bytes_moved):
            fn(); ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / reps
            return ms, bytes_moved / (ms * 1e-3) / 1e9

        copy_ms, copy_gbs = timed(lambda: ctx.check(ctx.lib.urt_buffer_set_data_device(ctx._h, big.handle, 0, src.data_ptr(), big_n)), 2 * 12 * big_n)
        nt, ne, nv = info["n_triangles"], info["n_entries"], info["count"]
        face_bytes, vertex_bytes = rate_bytes(nv, nt, ne)
        ms, gbs = timed(lambda: plan.compute(D), face_bytes + vertex_bytes)
        r = {"part": "rate", "vertices": nv, "triangles": nt, "entries": ne, "max_valence": info["max_valence"], "plan_ms": round(plan_ms, 1),
             "copy_elements": big_n, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1),
             "face_bytes": face_bytes, "vertex_bytes": vertex_bytes, "compute_normals_ms": round(ms, 4),
             "compute_normals_GBps": round(gbs, 1), "compute_normals_of_copy": round(gbs / copy_gbs, 3)}
        print(json.dumps(r), flush=True); results.append(r)
        plan.Release()
        for b in (V, I, D, big):
            b.Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels,update,rate")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    parts = args.part.split(",")
    if "kernels" in parts:
        part_kernels(args, results)
    if "update" in parts:
        part_update(args, results)
    if "rate" in parts:
        part_rate(args, results)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
