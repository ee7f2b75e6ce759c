# Scene-preparation time (SetData -> ready device scene, host wall clock reported by the library) for the reference's dynamic-scene
# protocol (RM:215-230: any move re-uploads EVERY buffer): nothing moved / one MeshObject moved / all moved, with the host SAH builder
# (per-MeshObject BVH cache) and with the three GPU builders (1 Karras radix tree, 2 depth-budgeted radix tree, 3 binned SAH).   python scripts/dynamic_scene.py [C4 C5]
# --move-objects: instead, RayTraceMaster.MoveObjects with temporal accumulation on (default builder): the whole step from the edits to the
# reprojected history (previous feature buffers, re-upload + refit, current feature buffers, motion tables, urt_reproject_objects), host wall
# clock to GPU-done, for one MeshObject moved and for all of them, and the share of the image that keeps its history.
import sys, time
sys.path.insert(0, '.')
import numpy as np
from unityraytracer_amd import Context, RayTraceMaster, scenes
ctx = Context(0)
names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["C4", "C5"]
if "--move-objects" in sys.argv:
    # --device-heaps: RayTraceMaster.device_object_heaps on (the object-level heaps are built on the GPU); --alternate: off and on, move by
    # move, in one process; --repeats N (default 1): N moves per label and form, each to a new place, reported as median [min .. max]
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 1
    names = [a for a in names if not a.isdigit()] or ["C4", "C5"]
    forms = (False, True) if "--alternate" in sys.argv else (True,) if "--device-heaps" in sys.argv else (False,)
    for name in names:
        sc = scenes.CONFIGS[name](640, 360)
        m = RayTraceMaster(ctx, sc)
        m.EnableTemporalAccumulation()
        for _ in range(8):
            m.OnRenderImage()
        ctx.synchronize()
        out, step = [], 0
        for label, ks in (("one moved", [len(sc.mesh_objects) - 1]), ("all moved", range(len(sc.mesh_objects))), ("all moved again", range(len(sc.mesh_objects)))):
            t = {f: [] for f in forms}
            for rep in range(repeats):
                for on in forms:
                    m.device_object_heaps = on
                    step += 1
                    edits = {}
                    for k in ks:
                        mat = np.asarray(sc.mesh_objects[k]["localToWorldMatrix"], np.float32).copy()
                        mat[12] += 0.05 if repeats == 1 else 0.01 * step
                        edits[k] = mat
                    t0 = time.perf_counter()
                    m.MoveObjects(edits)
                    t_host = (time.perf_counter() - t0) * 1e3
                    ctx.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3
                    kept = float((m._tcount.GetPixels()[..., 0] > 0).mean())
                    t[on].append((t_host, wall, kept))
                    for _ in range(4):
                        m.OnRenderImage()
                    ctx.synchronize()
            for on in forms:
                host, wall, kept = (np.array(c) for c in zip(*t[on]))
                tag = "heaps on the device" if on else "heaps on the host"
                if repeats == 1:
                    out.append(f"{label} ({tag}): host {host[0]:.1f} ms, edits-to-GPU-done {wall[0]:.1f} ms, {kept[0]:.3f} of the pixels keep history")
                else:
                    out.append(f"{label} ({tag}, {repeats} moves): host median {np.median(host):.2f} ms [{host.min():.2f} .. {host.max():.2f}], "
                               f"edits-to-GPU-done median {np.median(wall):.2f} ms [{wall.min():.2f} .. {wall.max():.2f}], {np.median(kept):.3f} of the pixels keep history")
        print(f"{name} {sc.n_triangles} triangles, {len(sc.mesh_objects)} MeshObjects, 640x360, MoveObjects with temporal accumulation: " + "; ".join(out), flush=True)
        m.OnDisable()
    sys.exit(0)
for name in names:
    sc = scenes.CONFIGS[name](640, 360)
    for builder in (0, 1, 2, 3):
        ctx.set_option("blas_builder", builder)
        m = RayTraceMaster(ctx, sc)
        m.OnRenderImage(); first = ctx.scene_info()["prepare_ms"]
        tag = []
        def reupload(mo):
            lo, hi = scenes.mesh_bounds(mo, sc.vertices, sc.indices)
            bvh = scenes.build_object_bvh(lo, hi)
            p0 = ctx.refit_stats()[1]
            t0 = time.perf_counter()
            for buf, data in ((m._meshObjectBuffer, mo), (m._vertexBuffer, sc.vertices), (m._indexBuffer, sc.indices), (m._normalBuffer, sc.normals), (m._meshObjectBVHBuffer, bvh)):
                buf.SetData(data)
            t_set = (time.perf_counter() - t0) * 1e3
            ms = ctx.scene_info()["prepare_ms"]
            ctx.synchronize()                                                     # the refit kernels are stream-ordered: include them in the wall time
            wall = (time.perf_counter() - t0) * 1e3
            tag.append(f"SetData x5 {t_set:.1f} ms, SetData-to-GPU-done {wall:.1f} ms" + (", in place" if ctx.refit_stats()[1] > p0 else ""))
            return ms
        same = min(reupload(sc.mesh_objects) for _ in range(3))
        one = sc.mesh_objects.copy()
        mat = np.asarray(one[-1]["localToWorldMatrix"], np.float32).copy(); mat[12] += 0.1; one[-1]["localToWorldMatrix"] = mat
        r0, b0 = ctx.blas_cache_stats()
        t_one = reupload(one)
        r1, b1 = ctx.blas_cache_stats()
        allm = sc.mesh_objects.copy()
        for k in range(len(allm)):
            mat = np.asarray(allm[k]["localToWorldMatrix"], np.float32).copy(); mat[12] += 0.05 * (k + 1); allm[k]["localToWorldMatrix"] = mat
        t_all = reupload(allm)
        print(f"{name} {sc.n_triangles} triangles, {len(sc.mesh_objects)} MeshObjects, builder {('host SAH', 'GPU Karras tree', 'GPU depth-budgeted tree', 'GPU binned SAH')[builder]}: first {first:.1f} ms; "
              f"re-upload unchanged: not stale ({tag[0]}); one moved {t_one:.2f} ms [{tag[3]}]" + (f" ({b1 - b0} built, {r1 - r0} reused)" if not builder else "") + f"; all moved {t_all:.2f} ms [{tag[4]}]", flush=True)
        m.OnDisable()
ctx.set_option("blas_builder", -1)
