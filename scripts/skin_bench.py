"""Cost of an animated mesh, from the first call of an update to the finished in-place update of the scene, three ways:
  (a) the host path: vertices and normals skinned on the host (its time is reported apart, `host_skin_ms`), then SetData of _Vertices,
      _Normals and _MeshBVH and the preparation — what a host had to do before the buffers had a device side.  `--parent-lib` runs this
      part on the parent commit's library too, in a child process in the same session;
  (b) the device path: RayTraceMaster.SkinMeshes — bones SetData + urt_skin_vertices + urt_buffer_bounds, the heap rebuilt from the
      returned bounds and SetData — and the preparation.  `--parent-lib` runs this part on the parent commit's library too;
  (b') the same with RayTraceMaster.device_object_heaps: urt_mesh_leaf_bounds_device + urt_build_object_bvh_device instead of the
      bounds calls and the host's heap — no synchronising call before the preparation.  (b) and (b') alternate, update by update;
  (c) positions that already live on the GPU: urt_buffer_set_data_device from torch tensors, SetData of _MeshBVH, the preparation.
Cases: C3's blob (one MeshObject, 34,802 vertices, 1920x1080), C5 with one and with all twelve MeshObjects skinned; every update is another
two-bone bend.  After the updates of (a) and of (b) with one and the same pose, the time of a 16-frame launch: the same tree, so the
same frame time.  Part `rate`: k_skin on 8 M vertices (0.5 - 0.7 GB touched) and k_bounds on 32 M (0.4 GB) as a fraction of the
device-to-device copy rate (bytes read + written per second) measured here with urt_buffer_set_data_device on 32 M elements — every
working set larger than the chip's 256 MB last-level cache.

    python scripts/skin_bench.py [--part update,rate] [--repeats 5] [--parent-lib old.so] [--json out.json]
"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process, tests/conftest.py)

import skin_ref as S  # noqa: E402  (the numpy restatement doubles as the host's skinning pass)
from unityraytracer_amd import ComputeBuffer, Context, RayTraceMaster, scenes  # noqa: E402

F = np.float32


def spans(sc):
    out = []
    for mo in sc.mesh_objects:
        sl = sc.indices[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"])]
        out.append((int(sl.min()), int(sl.max()) + 1))
    return out


def summary(name, ms):
    med = float(np.median(ms))
    return {name: [round(x, 3) for x in ms], name + "_median": round(med, 3), name + "_spread_pct": round(float((max(ms) - min(ms)) / med * 100), 1) if med > 0 else 0.0}


def launch_ms(ctx, m, frames=16):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        m.OnRenderImage()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def finish(ctx):
    ms = ctx.scene_info()["prepare_ms"]                      # prepares the stale scene
    ctx.synchronize()
    return ms


class Case:
    def __init__(self, sc, meshes):
        self.sc, self.meshes, self.sp = sc, meshes, spans(sc)
        self.skin = {k: S.two_bone_bend(sc.vertices[self.sp[k][0]: self.sp[k][1]], 30.0)[:2] for k in meshes}

    def bones(self, k, step):
        a, b = self.sp[k]
        return S.two_bone_bend(self.sc.vertices[a:b], 12.0 + 7.0 * step + k)[2]

    def host_skin(self, step):
        """-> (vertices, normals, ms of the host's skinning pass)"""
        v, n = self.sc.vertices.copy(), self.sc.normals.copy()
        t0 = time.perf_counter()
        for k in self.meshes:
            a, b = self.sp[k]
            v[a:b], n[a:b] = S.skin(self.sc.vertices[a:b], self.sc.normals[a:b], *self.skin[k], self.bones(k, step))
        return v, n, (time.perf_counter() - t0) * 1e3


def update_host(ctx, m, v, n, heap):
    ctx.synchronize()
    t0 = time.perf_counter()
    m._vertexBuffer.SetData(v)
    m._normalBuffer.SetData(n)
    m._meshObjectBVHBuffer.SetData(heap)
    t1 = time.perf_counter()
    finish(ctx)
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3


def part_update(args, tag, results):
    device_side = tag != "parent"
    for cfg, size, which in (("C3", (1920, 1080), "one"), ("C5", (640, 360), "one"), ("C5", (640, 360), "all")):
        sc = scenes.CONFIGS[cfg](*size)
        n = len(sc.mesh_objects)
        meshes = [n - 1] if which == "one" else list(range(n))
        case = Case(sc, meshes)
        poses = [case.host_skin(s + 1) for s in range(args.repeats + 1)]
        heaps = [scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices)) for v, _, _ in poses]
        base = {"lib": tag, "part": "update", "config": cfg, "triangles": sc.n_triangles, "meshes": n, "skinned_per_update": len(meshes),
                "skinned_vertices": int(sum(case.sp[k][1] - case.sp[k][0] for k in meshes))}
        with Context(0) as ctx:
            m = RayTraceMaster(ctx, copy.copy(sc))
            m.OnRenderImage()
            ctx.synchronize()
            # (a) the host path
            t = [update_host(ctx, m, v, nr, h) for (v, nr, _), h in zip(poses, heaps)][1:]      # the first one warms up
            r = dict(base, path="a_host_set_data")
            r.update(summary("host_skin_ms", [p[2] for p in poses[1:]]))
            r.update(summary("set_data_ms", [x[0] for x in t]))
            r.update(summary("update_ms", [x[1] for x in t]))
            r.update(summary("launch16_ms", [launch_ms(ctx, m) for _ in range(3)]))
            print(json.dumps(r), flush=True); results.append(r)
            # (b) the device path, ending on the pose (a) ended on, and (b') the same with the heaps built on the device: they alternate
            for k in meshes:
                m.AttachSkin(k, *case.skin[k])
            m._vertexBuffer.SetData(sc.vertices); m._normalBuffer.SetData(sc.normals); finish(ctx)
            t = {False: [], True: []}
            bone_sets = [{k: case.bones(k, s + 1) for k in meshes} for s in range(args.repeats + 1)]      # (what an animation system hands over)
            forms = (False, True) if device_side else (False,)                    # (the parent's library has no device heaps)
            for bones in bone_sets:
                for on in forms:
                    m.device_object_heaps = on
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    m.SkinMeshes(bones)
                    finish(ctx)
                    t[on].append((time.perf_counter() - t0) * 1e3)
            m.device_object_heaps = False
            m.SkinMeshes(bone_sets[-1]); finish(ctx)                              # (the launch below: on the host path's heap, as before)
            r = dict(base, path="b_skin_on_device")
            r.update(summary("update_ms", t[False][1:]))
            r.update(summary("launch16_ms", [launch_ms(ctx, m) for _ in range(3)]))
            r["downloads"] = ctx.buffer_state(m._vertexBuffer)["downloads"] + ctx.buffer_state(m._normalBuffer)["downloads"]
            r["in_place"] = ctx.deform_stats()["deformed"]
            print(json.dumps(r), flush=True); results.append(r)
            if not device_side:
                m.OnDisable()
                continue
            m.device_object_heaps = True
            m.SkinMeshes(bone_sets[-1]); finish(ctx)
            r = dict(base, path="b2_skin_on_device_heaps_on_device")
            r.update(summary("update_ms", t[True][1:]))
            r.update(summary("launch16_ms", [launch_ms(ctx, m) for _ in range(3)]))
            r["downloads"] = ctx.buffer_state(m._vertexBuffer)["downloads"] + ctx.buffer_state(m._normalBuffer)["downloads"]
            r["heap_downloads"] = ctx.buffer_state(m._meshObjectBVHBuffer)["downloads"]
            print(json.dumps(r), flush=True); results.append(r)
            m.device_object_heaps = False
            # (c) positions that live in torch tensors
            lo, hi = min(case.sp[k][0] for k in meshes), max(case.sp[k][1] for k in meshes)
            dev = [(torch.from_numpy(v[lo:hi]).cuda(), torch.from_numpy(nr[lo:hi]).cuda()) for v, nr, _ in poses]
            torch.cuda.synchronize()
            t = []
            for (tv, tn), h in zip(dev, heaps):
                ctx.synchronize()
                t0 = time.perf_counter()
                m._vertexBuffer.SetDataDevice(tv, lo)
                m._normalBuffer.SetDataDevice(tn, lo)
                m._meshObjectBVHBuffer.SetData(h)
                finish(ctx)
                t.append((time.perf_counter() - t0) * 1e3)
            r = dict(base, path="c_set_data_device")
            r.update(summary("update_ms", t[1:]))
            r["downloads"] = ctx.buffer_state(m._vertexBuffer)["downloads"] + ctx.buffer_state(m._normalBuffer)["downloads"]
            print(json.dumps(r), flush=True); results.append(r)
            m.OnDisable()


def part_rate(args, results):
    n, big_n, reps = 8 << 20, 32 << 20, 30
    rng = np.random.default_rng(0)
    with Context(0) as ctx:
        bufs = {k: ComputeBuffer(ctx, n, s) for k, s in (("rest_v", 12), ("rest_n", 12), ("idx", 16), ("wgt", 16), ("dst_v", 12), ("dst_n", 12))}
        bufs["rest_v"].SetData(rng.uniform(-1, 1, (n, 3)).astype(F)); bufs["rest_n"].SetData(rng.normal(size=(n, 3)).astype(F))
        w = rng.uniform(0, 1, (n, 4)).astype(F)
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
        r = {"part": "rate", "skin_vertices": n, "copy_and_bounds_elements": big_n, "copy_ms": round(copy_ms, 4), "copy_GBps": round(copy_gbs, 1)}
        for n_bones in (64, 1024):                            # staged in LDS / gathered from global memory
            bones = ComputeBuffer(ctx, n_bones, 48)
            bones.SetData(rng.uniform(-1, 1, (n_bones, 12)).astype(F))
            bufs["idx"].SetData(rng.integers(0, n_bones, (n, 4)).astype(np.int32)); bufs["wgt"].SetData(w)
            for normals, bytes_per in ((True, 12 + 12 + 16 + 16 + 12 + 12), (False, 12 + 16 + 16 + 12)):
                ms, gbs = timed(lambda: ctx.skin_vertices(bufs["rest_v"], bufs["rest_n"] if normals else None, bufs["idx"], bufs["wgt"], bones, 0, n,
                                                          bufs["dst_v"], bufs["dst_n"] if normals else None), bytes_per * n)
                key = f"skin_{n_bones}_bones_{'normals' if normals else 'positions'}"
                r.update({key + "_ms": round(ms, 4), key + "_GBps": round(gbs, 1), key + "_of_copy": round(gbs / copy_gbs, 3)})
            bones.Release()
        ms, gbs = timed(lambda: ctx.buffer_bounds(big), 12 * big_n)            # (every call waits: the time includes the synchronisation)
        r.update({"bounds_ms": round(ms, 4), "bounds_GBps": round(gbs, 1), "bounds_of_copy": round(gbs / copy_gbs, 3)})
        print(json.dumps(r), flush=True); results.append(r)
        for b in list(bufs.values()) + [big]:
            b.Release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="update,rate")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library: path (a) on it, in a child process")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = []
    if args.parent_lib:
        env = dict(os.environ, URT_LIB_PATH=os.path.abspath(args.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "update", "--tag", "parent", "--repeats", str(args.repeats)],
                             env=env, check=True, capture_output=True, text=True, timeout=600).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                results.append(json.loads(line))
    parts = args.part.split(",")
    if "update" in parts:
        part_update(args, args.tag, results)
    if "rate" in parts:
        part_rate(args, results)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
