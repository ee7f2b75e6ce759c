"""Cost of a mesh that changes SHAPE (include/urt.h option "refit_vertices"): the in-place update of changed _Vertices / _Normals against
the full preparation of the same change, and the sweep that decides the default of option "refit_rebuild_pct".

Parts (each prints one JSON line per case):
  update  C3 (one MeshObject, 69,600 triangles, 1920x1080) and C5 (12 MeshObjects, 983,040 triangles), one MeshObject deformed per update
          and all of them: the host time of SetData (compare + copy of _Vertices, _Normals, _MeshBVH) and of the scene preparation that
          follows (`prepare_ms`: urt_debug_scene_info, waited for), `--repeats` updates each, every one a new shape.  Run on a library
          without the in-place path — the parent commit's, through --parent-lib, in a child process on the same box — the same protocol
          measures the full preparation of the same changes.
  sweep   the C3 blob deformed away from the shape its tree was built for, by growing `phase` and `bumps` steps.  Per step: the cost ratio
          of the refitted tree (urt_debug_deform_stats), the host time of a 64-frame launch on the refitted tree and on a tree rebuilt from
          scratch for the same shape (alternating, `--repeats` each), and the in-place update time against the parent's full preparation.
          Break-even for a host that deforms every frame and renders one frame per deformation: extra frame time on the refitted tree
          >= full preparation time - update time.
The kernels' share: `k_refit_norms` gathers 36 B and writes 48 B per triangle, `k_tree_cost` reads 64 B per node; their times come from a
separate `rocprofv3 --kernel-trace --stats` run of `--part update`.

    python scripts/deform_bench.py [--part update,sweep] [--repeats 5] [--parent-lib old.so] [--json out.json]
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

import torch  # noqa: E402,F401  (before the library: one HIP runtime in the process, tests/conftest.py)

from unityraytracer_amd import Context, RayTraceMaster, host_scene, scenes  # noqa: E402

SWEEP = [(0.5 * k, 0.12 + 0.08 * k) for k in range(1, 8)]        # (phase, bumps) of the C3 blob, step by step further from (0, 0.12)


def spans(sc):
    out = []
    for mo in sc.mesh_objects:
        sl = sc.indices[int(mo["indices_offset"]): int(mo["indices_offset"]) + int(mo["indices_count"])]
        out.append((int(sl.min()), int(sl.max()) + 1))
    return out


def wobbled(sc, meshes, step):
    """The scene with the vertices of `meshes` displaced radially by a few percent (another shape for every step), normals and heap redone."""
    out = copy.copy(sc)
    v = sc.vertices.copy()
    sp = spans(sc)
    for k in meshes:
        a, b = sp[k]
        p = sc.vertices[a:b].astype(np.float64)
        v[a:b] = (p * (1.0 + 0.03 * np.sin(5.0 * p[:, 1:2] + 3.0 * p[:, 0:1] + 0.7 * step))).astype(np.float32)
    out.vertices = v
    out.normals = host_scene.compute_normals(v, sc.indices)
    out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices))
    return out


def blob_shape(sc, phase, bumps):
    out = copy.copy(sc)
    v, _ = scenes.uv_blob(200, 175, bumps=bumps, phase=phase)
    out.vertices = v
    out.normals = host_scene.compute_normals(v, sc.indices)
    out.mesh_bvh = scenes.build_object_bvh(*scenes.mesh_bounds(sc.mesh_objects, v, sc.indices))
    return out


def set_shape(ctx, m, sc):
    """SetData of what a deformation changes, then the preparation.  -> (SetData ms, prepare ms), host wall time."""
    ctx.synchronize()
    t0 = time.perf_counter()
    m._vertexBuffer.SetData(sc.vertices)
    m._normalBuffer.SetData(sc.normals)
    m._meshObjectBVHBuffer.SetData(sc.mesh_bvh)
    t1 = time.perf_counter()
    ms = ctx.scene_info()["prepare_ms"]
    ctx.synchronize()
    return (t1 - t0) * 1e3, ms


def deform_stats(ctx):
    return ctx.deform_stats() if hasattr(ctx.lib, "urt_debug_deform_stats") else None


def summary(name, ms):
    med = float(np.median(ms))
    return {name: [round(x, 3) for x in ms], name + "_median": round(med, 3), name + "_spread_pct": round(float((max(ms) - min(ms)) / med * 100), 1) if med > 0 else 0.0}


def part_update(args, tag, results):
    for cfg, size in (("C3", (1920, 1080)), ("C5", (640, 360))):
        sc = scenes.CONFIGS[cfg](*size)
        n = len(sc.mesh_objects)
        with Context(0) as ctx:
            m = RayTraceMaster(ctx, sc)
            m.OnRenderImage()
            ctx.synchronize()
            first = ctx.scene_info()["prepare_ms"]
            for case, meshes in (("one", [n - 1]), ("all", list(range(n)))):
                if cfg == "C3" and case == "all":
                    continue                                         # (C3 has one MeshObject)
                shapes = [wobbled(sc, meshes, s + 1) for s in range(args.repeats + 1)]
                d0 = deform_stats(ctx)
                times = [set_shape(ctx, m, s) for s in shapes][1:]    # the first one warms up
                d1 = deform_stats(ctx)
                r = {"lib": tag, "part": "update", "config": cfg, "triangles": sc.n_triangles, "meshes": n, "deformed_per_update": len(meshes),
                     "builder": ctx.launch_info()["blas_builder"], "first_prepare_ms": round(first, 3)}
                r.update(summary("set_data_ms", [t[0] for t in times]))
                r.update(summary("prepare_ms", [t[1] for t in times]))
                if d0 is not None:
                    r["in_place_meshes"] = d1["deformed"] - d0["deformed"]
                    r["bytes_copied_per_update"] = (d1["bytes_copied"] - d0["bytes_copied"]) // (args.repeats + 1)
                print(json.dumps(r), flush=True)
                results.append(r)
            if cfg == "C3":                                          # the sweep's shapes, each from the base shape: what a full preparation of them costs
                for k, (phase, bumps) in enumerate(SWEEP):
                    shape = blob_shape(sc, phase, bumps)
                    ms = []
                    for _ in range(args.repeats):
                        set_shape(ctx, m, sc)
                        ms.append(set_shape(ctx, m, shape)[1])
                    r = {"lib": tag, "part": "sweep_prepare", "step": k, "phase": phase, "bumps": round(bumps, 2)}
                    r.update(summary("prepare_ms", ms))
                    print(json.dumps(r), flush=True)
                    results.append(r)
            m.OnDisable()


def launch_ms(ctx, m, frames=64):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        m.OnRenderImage()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def part_sweep(args, results, parent):
    sc = scenes.config3(1920, 1080)
    full = {r["step"]: r["prepare_ms_median"] for r in parent if r.get("part") == "sweep_prepare"}
    with Context(0) as ctx:
        m = RayTraceMaster(ctx, sc)
        launch_ms(ctx, m)

        def rebuilt(shape):
            """A tree built from scratch for `shape` (toggling "refit" asks for a full preparation)."""
            ctx.set_option("refit", 0); ctx.set_option("refit", 1)
            return set_shape(ctx, m, shape)[1]

        for k, (phase, bumps) in enumerate(SWEEP):
            shape = blob_shape(sc, phase, bumps)
            t_refit, t_built, upd, ratio = [], [], [], 0.0
            for _ in range(args.repeats):
                rebuilt(sc)                                          # the tree of the base shape ...
                upd.append(set_shape(ctx, m, shape)[1])              # ... refitted to this step's
                ratio = ctx.deform_stats()["cost_ratio"]
                launch_ms(ctx, m, 8)
                t_refit.append(launch_ms(ctx, m))
                rebuilt(shape)
                launch_ms(ctx, m, 8)
                t_built.append(launch_ms(ctx, m))
            r = {"part": "sweep", "step": k, "phase": phase, "bumps": round(bumps, 2), "cost_ratio": round(float(ratio), 4)}
            r.update(summary("launch64_refitted_ms", t_refit))
            r.update(summary("launch64_rebuilt_ms", t_built))
            r.update(summary("update_ms", upd))
            r["extra_frame_ms"] = round((r["launch64_refitted_ms_median"] - r["launch64_rebuilt_ms_median"]) / 64.0, 4)
            if k in full:
                r["parent_full_prepare_ms"] = full[k]
                r["saved_per_update_ms"] = round(full[k] - r["update_ms_median"], 3)
                r["break_even"] = bool(r["extra_frame_ms"] >= r["saved_per_update_ms"])
            print(json.dumps(r), flush=True)
            results.append(r)
        m.OnDisable()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="update,sweep")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library: its full preparations of the same changes, in a child process")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results, parent = [], []
    if args.parent_lib:
        env = dict(os.environ, URT_LIB_PATH=os.path.abspath(args.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "update", "--tag", "parent", "--repeats", str(args.repeats)],
                             env=env, check=True, capture_output=True, text=True, timeout=600).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                parent.append(json.loads(line))
    parts = args.part.split(",")
    if "update" in parts:
        part_update(args, args.tag, results)
    if "sweep" in parts:
        part_sweep(args, results, parent)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(parent + results, f, indent=1)


if __name__ == "__main__":
    main()
