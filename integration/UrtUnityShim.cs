// UrtUnityShim.cs — stand-ins with the SAME member names RayTraceMaster.cs ("RM") uses on UnityEngine.ComputeBuffer,
// ComputeShader, RenderTexture and Graphics.Blit, implemented over UrtNative (libunityraytracer_amd.so).  With this file in
// Assets/Scripts/, RM changes only type names at its declarations (RM:8, 11-12, 26-37: ComputeShader -> UrtComputeShader,
// ComputeBuffer -> UrtComputeBuffer, RenderTexture -> UrtRenderTexture) and the three Graphics.Blit calls of RM:818-819
// (-> UrtGraphics.Blit); every call inside its methods compiles unchanged against these classes.  Set UrtDevice.Devices to
// more than one ordinal and the same RM drives a device group: the frame is cut into 8-row strips over the GPUs and
// UrtGraphics.Blit(_converged, destination) performs the one frame-end gather.  SOURCE ONLY (no C# toolchain in the build
// image of this repository); the Python twin of this file, which IS exercised by tests, is unityraytracer_amd/unity_api.py.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using UnityEngine;

/// The process-wide device selection: one context, or a group when several ordinals are listed.
public static class UrtDevice {
    public static int[] Devices = { 0 };
    static IntPtr ctx = IntPtr.Zero, group = IntPtr.Zero;
    internal static bool IsGroup { get { Ensure(); return group != IntPtr.Zero; } }
    internal static IntPtr Handle { get { Ensure(); return group != IntPtr.Zero ? group : ctx; } }
    static void Ensure() {
        if (ctx != IntPtr.Zero || group != IntPtr.Zero) return;
        // a negative ABI version marks an A/B / probe / diagnostic BUILD of the library (csrc/experiments.h): never the product
        if (UrtNative.urt_abi_version() < 0) throw new InvalidOperationException("libunityraytracer_amd is an experiment build (negative urt_abi_version): refused");
        if (Devices.Length > 1) UrtNative.CheckGroup(IntPtr.Zero, UrtNative.urt_group_create(Devices, Devices.Length, out group));
        else UrtNative.Check(IntPtr.Zero, UrtNative.urt_context_create(Devices[0], out ctx));
    }
    internal static void Check(int rc) { if (IsGroup) UrtNative.CheckGroup(group, rc); else UrtNative.Check(ctx, rc); }
    public static void Shutdown() {
        if (group != IntPtr.Zero) UrtNative.urt_group_destroy(group);
        if (ctx != IntPtr.Zero) UrtNative.urt_context_destroy(ctx);
        group = ctx = IntPtr.Zero;
    }
}

/// Physics.Raycast-style queries against the scene the bound shader renders (include/urt.h urt_ray_query): picking, line of sight,
/// the "test ray" of RayTraceDebug.cs:119-129.  One context only (a group user queries urt_group_context(g, r)).
internal static class UrtRaycast {                   // internal: it hands out UrtNative records (same assembly as RM)
    static readonly UrtNative.Ray[] one = new UrtNative.Ray[1];
    static readonly UrtNative.RayHit[] oneHit = new UrtNative.RayHit[1];
    public static bool Raycast(Vector3 origin, Vector3 direction, out UrtNative.RayHit hit, float maxDistance = float.PositiveInfinity) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("Raycast: query one rank's context (urt_group_context)");
        one[0] = new UrtNative.Ray { ox = origin.x, oy = origin.y, oz = origin.z, tMax = maxDistance, dx = direction.x, dy = direction.y, dz = direction.z };
        UrtDevice.Check(UrtNative.urt_ray_query(UrtDevice.Handle, one, 1, oneHit, UrtNative.QueryClosest));
        hit = oneHit[0];
        return hit.kind != 0;
    }
    /// Occlusion of many segments at once: occluded[i] = 1 if anything lies strictly between 0 and rays[i].tMax.
    public static void Occluded(UrtNative.Ray[] rays, int[] occluded) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("Occluded: query one rank's context (urt_group_context)");
        UrtDevice.Check(UrtNative.urt_ray_query_any(UrtDevice.Handle, rays, rays.Length, occluded, UrtNative.QueryAny));
    }
}

/// Path-traced radiance outside a frame (include/urt.h urt_radiance_query): light probes / lightmap texels (SampleRadiance) and fresh
/// samples for chosen pixels of the bound camera, e.g. the ones a reprojection left without history (ResamplePixels).  Results are
/// RGBA floats, four per query.  One context only (a group user queries urt_group_context(g, r)).
internal static class UrtRadiance {                  // internal: it takes UrtNative records (same assembly as RM)
    /// rays[i].seed and (px, py) select each query's random stream; samples 1..4096 paths of up to `bounces` (0..64) bounces each.
    public static void SampleRadiance(UrtNative.PathRay[] rays, int samples, int bounces, float[] outRgba) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("SampleRadiance: query one rank's context (urt_group_context)");
        if (outRgba.Length < 4 * rays.Length) throw new ArgumentException("SampleRadiance: outRgba holds fewer than 4 floats per ray");
        UrtDevice.Check(UrtNative.urt_radiance_query(UrtDevice.Handle, rays, rays.Length, samples, bounces, outRgba, UrtNative.RadianceRays));
    }
    /// What a frame dispatched now with _numRays = samples and _numBounces = bounces would write to the pixels (of the texture bound as Result).
    public static void ResamplePixels(UrtNative.PathPixel[] pixels, int samples, int bounces, float[] outRgba) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("ResamplePixels: query one rank's context (urt_group_context)");
        if (outRgba.Length < 4 * pixels.Length) throw new ArgumentException("ResamplePixels: outRgba holds fewer than 4 floats per pixel");
        UrtDevice.Check(UrtNative.urt_radiance_query_pixels(UrtDevice.Handle, pixels, pixels.Length, samples, bounces, outRgba, UrtNative.RadiancePixels));
    }
}

/// Per-pixel first-hit feature buffers (include/urt.h urt_render_aov) written straight into device memory the engine owns — how a Unity
/// RenderTexture (ARGBFloat, enableRandomWrite) is bound: pass each texture's device pointer (GetNativeTexturePtr on a HIP-interop
/// backend) or IntPtr.Zero for a buffer not wanted.  Call it when the camera moves, after SetShaderParameters (the accumulation resets then too).
public static class UrtFeatureBuffers {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly ulong[] handles = new ulong[4];
    static readonly IntPtr[] ptrs = new IntPtr[4];
    static int w, h;
    public static void Render(IntPtr hit, IntPtr normal, IntPtr albedo, IntPtr id, int width, int height, bool frameRay = false) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtFeatureBuffers: render on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        IntPtr[] want = { hit, normal, albedo, id };
        for (int k = 0; k < 4; k++) {                                  // the external textures are re-wrapped when a pointer or the size changes
            if (handles[k] != 0 && (boundCtx != ctx || ptrs[k] != want[k] || w != width || h != height)) {
                if (boundCtx == ctx) UrtDevice.Check(UrtNative.urt_texture_release(ctx, handles[k]));
                handles[k] = 0;
            }
            if (handles[k] == 0 && want[k] != IntPtr.Zero)
                UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, want[k], out handles[k]));
            ptrs[k] = want[k];
        }
        boundCtx = ctx; w = width; h = height;
        UrtDevice.Check(UrtNative.urt_render_aov(ctx, handles[0], handles[1], handles[2], handles[3],
                                                 frameRay ? UrtNative.AovFrameRay : UrtNative.AovPixelCenter));
    }
}

/// Edge-aware denoise (include/urt.h urt_denoise) of device images the engine owns: the accumulated image `src` (RM:12 _converged's
/// RenderTexture), the output `dst` (may be src) and the hit / normal / albedo feature buffers UrtFeatureBuffers.Render wrote
/// (IntPtr.Zero albedo = no demodulation), all ARGBFloat of one size.  Call it every frame before the present; refresh the guides with
/// UrtFeatureBuffers.Render when the camera moves (the accumulation resets then too).  Defaults: include/urt.h URT_DENOISE_DEFAULT_*.
public static class UrtDenoiser {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly ulong[] handles = new ulong[5];
    static readonly IntPtr[] ptrs = new IntPtr[5];
    static int w, h;
    public static void Denoise(IntPtr src, IntPtr dst, IntPtr hit, IntPtr normal, IntPtr albedo, int width, int height,
                               int iterations = 5, float sigmaColor = 8.0f, float sigmaNormal = 0.5f, float sigmaDepth = 0.1f) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtDenoiser: denoise on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        IntPtr[] want = { src, dst, hit, normal, albedo };
        for (int k = 0; k < 5; k++) {                                  // the external textures are re-wrapped when a pointer or the size changes
            if (handles[k] != 0 && (boundCtx != ctx || ptrs[k] != want[k] || w != width || h != height)) {
                if (boundCtx == ctx) UrtDevice.Check(UrtNative.urt_texture_release(ctx, handles[k]));
                handles[k] = 0;
            }
            if (handles[k] == 0 && want[k] != IntPtr.Zero && !(k == 1 && want[1] == want[0]))
                UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, want[k], out handles[k]));
            ptrs[k] = want[k];
        }
        boundCtx = ctx; w = width; h = height;
        ulong dstHandle = dst == src ? handles[0] : handles[1];           // in place: one handle for both
        var p = new UrtNative.DenoiseParams { iterations = iterations, sigmaColor = sigmaColor, sigmaNormal = sigmaNormal, sigmaDepth = sigmaDepth };
        UrtDevice.Check(UrtNative.urt_denoise(ctx, handles[0], dstHandle, handles[2], handles[3], handles[4], in p));
    }
}

/// Temporal accumulation (include/urt.h urt_reproject / urt_blit_add_history) over device images the engine owns, all ARGBFloat of one
/// size.  Per camera move: keep the previous camera's `prevViewProj` (_camera.projectionMatrix * _camera.worldToCameraMatrix) and its
/// pixel-centre feature buffers (UrtFeatureBuffers.Render into a second set), render the new camera's, then Reproject the accumulated
/// image and its count texture into a spare pair and swap.  Per frame: BlitAddHistory(_target, _converged, count) in place of the
/// AdditionShader blit.  A count texture starts as zeros (write them; creation is not assumed to zero).  Defaults: include/urt.h
/// URT_REPROJECT_DEFAULT_*.
public static class UrtTemporal {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly Dictionary<IntPtr, ulong> wrapped = new Dictionary<IntPtr, ulong>();
    static int w, h;
    static ulong Wrap(IntPtr ctx, IntPtr p, int width, int height) {  // external textures, re-wrapped when the context or the size changes
        if (p == IntPtr.Zero) return 0;
        if (boundCtx != ctx || w != width || h != height) {
            if (boundCtx == ctx) foreach (ulong t in wrapped.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
            wrapped.Clear();
            boundCtx = ctx; w = width; h = height;
        }
        if (!wrapped.TryGetValue(p, out ulong handle)) {
            UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, p, out handle));
            wrapped[p] = handle;
        }
        return handle;
    }
    public static void Reproject(IntPtr prevColor, IntPtr prevCount, IntPtr prevHit, IntPtr prevNormal, IntPtr prevId,
                                 IntPtr hit, IntPtr normal, IntPtr id, IntPtr color, IntPtr count, IntPtr motion, int width, int height,
                                 Matrix4x4 prevViewProj, float maxHistory = 64.0f, float normalThreshold = 0.9f, float planeThreshold = 0.02f) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtTemporal: reproject on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var m = new float[16];
        for (int k = 0; k < 16; k++) m[k] = prevViewProj[k];          // Matrix4x4's indexer is column-major: the order of the ABI
        var im = new UrtNative.ReprojectImages {
            prevColor = Wrap(ctx, prevColor, width, height), prevCount = Wrap(ctx, prevCount, width, height),
            prevHit = Wrap(ctx, prevHit, width, height), prevNormal = Wrap(ctx, prevNormal, width, height), prevId = Wrap(ctx, prevId, width, height),
            hit = Wrap(ctx, hit, width, height), normal = Wrap(ctx, normal, width, height), id = Wrap(ctx, id, width, height),
            color = Wrap(ctx, color, width, height), count = Wrap(ctx, count, width, height), motion = Wrap(ctx, motion, width, height) };
        var p = new UrtNative.ReprojectParams { prevWorldToClip = m, maxHistory = maxHistory, normalThreshold = normalThreshold,
                                                planeThreshold = planeThreshold, flags = 0 };
        UrtDevice.Check(UrtNative.urt_reproject(ctx, in im, in p));
    }
    // ---- objects that move (include/urt.h urt_reproject_objects) ----
    static ulong meshTable, sphereTable;
    static int meshTableCount, sphereTableCount;
    static IntPtr tableCtx = IntPtr.Zero;
    // the motion table of one kind of object: urt_host_*_motion over the pinned previous and current lists -> a stride-48 buffer
    static ulong Table<T>(IntPtr ctx, List<T> prev, List<T> cur, bool mesh, ref ulong handle, ref int count) where T : struct {
        if (prev == null || cur == null || cur.Count == 0) return 0;
        if (prev.Count != cur.Count) throw new ArgumentException("UrtTemporal.MoveObjects: the previous and the current list differ in length");
        int n = cur.Count;
        var table = new float[12 * n];
        GCHandle a = GCHandle.Alloc(prev.ToArray(), GCHandleType.Pinned), b = GCHandle.Alloc(cur.ToArray(), GCHandleType.Pinned),
                 o = GCHandle.Alloc(table, GCHandleType.Pinned);
        try {
            int rc = mesh ? UrtNative.urt_host_mesh_motion(a.AddrOfPinnedObject(), b.AddrOfPinnedObject(), n, o.AddrOfPinnedObject())
                          : UrtNative.urt_host_sphere_motion(a.AddrOfPinnedObject(), b.AddrOfPinnedObject(), n, o.AddrOfPinnedObject());
            if (rc != 0) throw new InvalidOperationException("urt_host_" + (mesh ? "mesh" : "sphere") + "_motion: " +
                                                             Marshal.PtrToStringAnsi(UrtNative.urt_host_last_error()));
            if (handle != 0 && (tableCtx != ctx || count != n)) {
                if (tableCtx == ctx) UrtDevice.Check(UrtNative.urt_buffer_release(ctx, handle));
                handle = 0;
            }
            if (handle == 0) UrtDevice.Check(UrtNative.urt_buffer_create(ctx, n, UrtNative.ObjectMotionStride, out handle));
            count = n;
            UrtDevice.Check(UrtNative.urt_buffer_set_data(ctx, handle, o.AddrOfPinnedObject(), n));
        } finally { a.Free(); b.Free(); o.Free(); }
        return handle;
    }
    /// Objects (and optionally the camera) move while the accumulated image is kept.  The steps of RayTraceMaster.MoveObjects of the Python
    /// mirror: (a) renderFeatureBuffers(prevHit, prevNormal, prevId) while the old scene and camera are still bound, (b) applyEdits(): the
    /// host changes its _meshObjects / _spheres, rebuilds the object-level heaps and re-uploads through SetData as RebuildTrees does, and
    /// sets the new camera matrices if the camera moves too, (c) renderFeatureBuffers(hit, normal, id), (d) the two tables from the lists
    /// before and after (a list pair that is null means no object of that kind has moved), (e) urt_reproject_objects.  prevViewProj is
    /// the projectionMatrix * worldToCameraMatrix the history was accumulated under.  The host then swaps (color, count) with its
    /// _converged / count pair as after Reproject.  MeshObject / Sphere are the host's own sequential structs (RM:82-86, RM:116-119).
    public static void MoveObjects<TMesh, TSphere>(List<TMesh> prevMeshObjects, List<TMesh> meshObjects, List<TSphere> prevSpheres, List<TSphere> spheres,
                                                   Action applyEdits, Action<IntPtr, IntPtr, IntPtr> renderFeatureBuffers,
                                                   IntPtr prevColor, IntPtr prevCount, IntPtr prevHit, IntPtr prevNormal, IntPtr prevId,
                                                   IntPtr hit, IntPtr normal, IntPtr id, IntPtr color, IntPtr count, IntPtr motion, int width, int height,
                                                   Matrix4x4 prevViewProj, float maxHistory = 64.0f, float normalThreshold = 0.9f, float planeThreshold = 0.02f,
                                                   float movedMaxHistory = 0.0f) where TMesh : struct where TSphere : struct {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtTemporal: reproject on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        List<TMesh> meshBefore = prevMeshObjects != null ? new List<TMesh>(prevMeshObjects) : null;      // copies: applyEdits may edit in place
        List<TSphere> spheresBefore = prevSpheres != null ? new List<TSphere>(prevSpheres) : null;
        renderFeatureBuffers(prevHit, prevNormal, prevId);                                               // (a)
        applyEdits();                                                                                    // (b)
        renderFeatureBuffers(hit, normal, id);                                                           // (c)
        var mo = new UrtNative.ReprojectMotion {                                                         // (d)
            meshMotion = Table(ctx, meshBefore, meshObjects, true, ref meshTable, ref meshTableCount),
            sphereMotion = Table(ctx, spheresBefore, spheres, false, ref sphereTable, ref sphereTableCount),
            movedMaxHistory = movedMaxHistory, flags = 0 };
        tableCtx = ctx;
        var m = new float[16];
        for (int k = 0; k < 16; k++) m[k] = prevViewProj[k];
        var im = new UrtNative.ReprojectImages {
            prevColor = Wrap(ctx, prevColor, width, height), prevCount = Wrap(ctx, prevCount, width, height),
            prevHit = Wrap(ctx, prevHit, width, height), prevNormal = Wrap(ctx, prevNormal, width, height), prevId = Wrap(ctx, prevId, width, height),
            hit = Wrap(ctx, hit, width, height), normal = Wrap(ctx, normal, width, height), id = Wrap(ctx, id, width, height),
            color = Wrap(ctx, color, width, height), count = Wrap(ctx, count, width, height), motion = Wrap(ctx, motion, width, height) };
        var p = new UrtNative.ReprojectParams { prevWorldToClip = m, maxHistory = maxHistory, normalThreshold = normalThreshold,
                                                planeThreshold = planeThreshold, flags = 0 };
        UrtDevice.Check(UrtNative.urt_reproject_objects(ctx, in im, in p, in mo));                       // (e)
    }
    /// Meshes change shape while the accumulated image is kept: RayTraceMaster.DeformMeshes of the Python mirror.  The steps of MoveObjects
    /// with applyEdits() writing the new positions (and normals) of the deformed meshes' vertex spans through the ranged SetData and
    /// re-uploading the rebuilt object-level heap; the library refits those meshes on the GPU (option "refit_vertices").  The motion table
    /// holds the identity for every MeshObject but the deformed ones, whose entries are all NaN: urt_reproject_objects defines that as "no
    /// history", so they restart at count 0, everything else keeps its history, and ResampleDisocclusions fills them.  (No per-vertex
    /// motion vectors.)  nMeshObjects: length of _meshObjects; deformed: the indices of the deformed MeshObjects.
    public static void DeformMeshes(int nMeshObjects, IEnumerable<int> deformed, Action applyEdits, Action<IntPtr, IntPtr, IntPtr> renderFeatureBuffers,
                                    IntPtr prevColor, IntPtr prevCount, IntPtr prevHit, IntPtr prevNormal, IntPtr prevId,
                                    IntPtr hit, IntPtr normal, IntPtr id, IntPtr color, IntPtr count, IntPtr motion, int width, int height,
                                    Matrix4x4 prevViewProj, float maxHistory = 64.0f, float normalThreshold = 0.9f, float planeThreshold = 0.02f) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtTemporal: reproject on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var table = new float[12 * nMeshObjects];
        for (int k = 0; k < nMeshObjects; k++) table[12 * k] = table[12 * k + 4] = table[12 * k + 8] = 1.0f;      // the exact identity: not moved
        foreach (int k in deformed) {
            if (k < 0 || k >= nMeshObjects) throw new ArgumentOutOfRangeException(nameof(deformed), "UrtTemporal.DeformMeshes: no such MeshObject");
            for (int j = 0; j < 12; j++) table[12 * k + j] = float.NaN;
        }
        renderFeatureBuffers(prevHit, prevNormal, prevId);
        applyEdits();
        renderFeatureBuffers(hit, normal, id);
        if (meshTable != 0 && (tableCtx != ctx || meshTableCount != nMeshObjects)) {
            if (tableCtx == ctx) UrtDevice.Check(UrtNative.urt_buffer_release(ctx, meshTable));
            meshTable = 0;
        }
        GCHandle o = GCHandle.Alloc(table, GCHandleType.Pinned);
        try {
            if (meshTable == 0) UrtDevice.Check(UrtNative.urt_buffer_create(ctx, nMeshObjects, UrtNative.ObjectMotionStride, out meshTable));
            meshTableCount = nMeshObjects;
            UrtDevice.Check(UrtNative.urt_buffer_set_data(ctx, meshTable, o.AddrOfPinnedObject(), nMeshObjects));
        } finally { o.Free(); }
        tableCtx = ctx;
        var mo = new UrtNative.ReprojectMotion { meshMotion = meshTable, sphereMotion = 0, movedMaxHistory = 0.0f, flags = 0 };
        var m = new float[16];
        for (int k = 0; k < 16; k++) m[k] = prevViewProj[k];
        var im = new UrtNative.ReprojectImages {
            prevColor = Wrap(ctx, prevColor, width, height), prevCount = Wrap(ctx, prevCount, width, height),
            prevHit = Wrap(ctx, prevHit, width, height), prevNormal = Wrap(ctx, prevNormal, width, height), prevId = Wrap(ctx, prevId, width, height),
            hit = Wrap(ctx, hit, width, height), normal = Wrap(ctx, normal, width, height), id = Wrap(ctx, id, width, height),
            color = Wrap(ctx, color, width, height), count = Wrap(ctx, count, width, height), motion = Wrap(ctx, motion, width, height) };
        var p = new UrtNative.ReprojectParams { prevWorldToClip = m, maxHistory = maxHistory, normalThreshold = normalThreshold,
                                                planeThreshold = planeThreshold, flags = 0 };
        UrtDevice.Check(UrtNative.urt_reproject_objects(ctx, in im, in p, in mo));
    }
    // ---- meshes that change shape and keep their history (include/urt.h urt_reproject_deformed) ----
    static ulong prevVertices, prevObjects, deformedFlags;
    static int prevVerticesCount, prevObjectsCount;
    static IntPtr deformCtx = IntPtr.Zero;
    /// DeformMeshes with keepHistory: RayTraceMaster.DeformMeshes(..., keep_history=True) of the Python mirror.  vertices, indices and
    /// meshObjects are the handles of the buffers bound as _Vertices, _Indices and _MeshObjects (nVertices and nMeshObjects their counts).
    /// Before applyEdits() the vertex buffer is copied on the device into a previous-positions buffer (urt_buffer_copy: no download) and
    /// _MeshObjects into its twin; the motion table then holds the identity for every MeshObject and the deformed ones are flagged, so
    /// their pixels look up where the points of their triangle were (per-vertex motion) and keep their history.  keepHistory false: the
    /// overload above, to the bit.
    public static void DeformMeshes(int nMeshObjects, IEnumerable<int> deformed, Action applyEdits, Action<IntPtr, IntPtr, IntPtr> renderFeatureBuffers,
                                    IntPtr prevColor, IntPtr prevCount, IntPtr prevHit, IntPtr prevNormal, IntPtr prevId,
                                    IntPtr hit, IntPtr normal, IntPtr id, IntPtr color, IntPtr count, IntPtr motion, int width, int height,
                                    Matrix4x4 prevViewProj, bool keepHistory, ulong vertices, int nVertices, ulong indices, ulong meshObjects,
                                    float maxHistory = 64.0f, float normalThreshold = 0.9f, float planeThreshold = 0.02f,
                                    float deformNormalThreshold = UrtNative.ReprojectDefaultDeformNormalThreshold) {
        if (!keepHistory) {
            DeformMeshes(nMeshObjects, deformed, applyEdits, renderFeatureBuffers, prevColor, prevCount, prevHit, prevNormal, prevId, hit, normal, id,
                         color, count, motion, width, height, prevViewProj, maxHistory, normalThreshold, planeThreshold);
            return;
        }
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtTemporal: reproject on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var table = new float[12 * nMeshObjects];
        var flags = new int[nMeshObjects];
        for (int k = 0; k < nMeshObjects; k++) table[12 * k] = table[12 * k + 4] = table[12 * k + 8] = 1.0f;      // the exact identity: not moved
        foreach (int k in deformed) {
            if (k < 0 || k >= nMeshObjects) throw new ArgumentOutOfRangeException(nameof(deformed), "UrtTemporal.DeformMeshes: no such MeshObject");
            flags[k] = 1;
        }
        if (deformCtx != ctx || prevVerticesCount != nVertices || prevObjectsCount != nMeshObjects) {
            if (deformCtx == ctx)
                foreach (ulong h in new[] { prevVertices, prevObjects, deformedFlags })
                    if (h != 0) UrtDevice.Check(UrtNative.urt_buffer_release(ctx, h));
            UrtDevice.Check(UrtNative.urt_buffer_create(ctx, nVertices, 12, out prevVertices));
            UrtDevice.Check(UrtNative.urt_buffer_create(ctx, nMeshObjects, 112, out prevObjects));
            UrtDevice.Check(UrtNative.urt_buffer_create(ctx, nMeshObjects, 4, out deformedFlags));
            prevVerticesCount = nVertices; prevObjectsCount = nMeshObjects; deformCtx = ctx;
        }
        renderFeatureBuffers(prevHit, prevNormal, prevId);
        UrtDevice.Check(UrtNative.urt_buffer_copy(ctx, vertices, 0, prevVertices, 0, nVertices));         // the scene as the history saw it
        UrtDevice.Check(UrtNative.urt_buffer_copy(ctx, meshObjects, 0, prevObjects, 0, nMeshObjects));
        applyEdits();
        renderFeatureBuffers(hit, normal, id);
        if (meshTable != 0 && (tableCtx != ctx || meshTableCount != nMeshObjects)) {
            if (tableCtx == ctx) UrtDevice.Check(UrtNative.urt_buffer_release(ctx, meshTable));
            meshTable = 0;
        }
        GCHandle o = GCHandle.Alloc(table, GCHandleType.Pinned), f = GCHandle.Alloc(flags, GCHandleType.Pinned);
        try {
            if (meshTable == 0) UrtDevice.Check(UrtNative.urt_buffer_create(ctx, nMeshObjects, UrtNative.ObjectMotionStride, out meshTable));
            meshTableCount = nMeshObjects;
            UrtDevice.Check(UrtNative.urt_buffer_set_data(ctx, meshTable, o.AddrOfPinnedObject(), nMeshObjects));
            UrtDevice.Check(UrtNative.urt_buffer_set_data(ctx, deformedFlags, f.AddrOfPinnedObject(), nMeshObjects));
        } finally { o.Free(); f.Free(); }
        tableCtx = ctx;
        var mo = new UrtNative.ReprojectMotion { meshMotion = meshTable, sphereMotion = 0, movedMaxHistory = 0.0f, flags = 0 };
        var de = new UrtNative.ReprojectDeform { prevVertices = prevVertices, indices = indices, prevMeshObjects = prevObjects, deformed = deformedFlags,
                                                 normalThreshold = deformNormalThreshold, flags = 0 };
        var m = new float[16];
        for (int k = 0; k < 16; k++) m[k] = prevViewProj[k];
        var im = new UrtNative.ReprojectImages {
            prevColor = Wrap(ctx, prevColor, width, height), prevCount = Wrap(ctx, prevCount, width, height),
            prevHit = Wrap(ctx, prevHit, width, height), prevNormal = Wrap(ctx, prevNormal, width, height), prevId = Wrap(ctx, prevId, width, height),
            hit = Wrap(ctx, hit, width, height), normal = Wrap(ctx, normal, width, height), id = Wrap(ctx, id, width, height),
            color = Wrap(ctx, color, width, height), count = Wrap(ctx, count, width, height), motion = Wrap(ctx, motion, width, height) };
        var p = new UrtNative.ReprojectParams { prevWorldToClip = m, maxHistory = maxHistory, normalThreshold = normalThreshold,
                                                planeThreshold = planeThreshold, flags = 0 };
        UrtDevice.Check(UrtNative.urt_reproject_deformed(ctx, in im, in p, in mo, in de));
    }
    public static void BlitAddHistory(IntPtr src, IntPtr dst, IntPtr count, int width, int height, float maxHistory = 64.0f) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtTemporal: blend on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        UrtDevice.Check(UrtNative.urt_blit_add_history(ctx, Wrap(ctx, src, width, height), Wrap(ctx, dst, width, height),
                                                       Wrap(ctx, count, width, height), maxHistory));
    }
    /// After Reproject (or MoveObjects): fresh samples for the pixels the reprojection left with a count below `below` (1: no history at
    /// all), traced and blended into `converged` and `count` on the GPU (include/urt.h urt_resample_below).  The Result texture, the camera
    /// matrices, _PixelOffset and _Seed are those bound at call time: set a fresh _Seed first, as for a frame.  samples / bounces: the
    /// frame's _numRays / _numBounces make a resampled pixel exactly one frame's worth (weight 1).  Returns the number of pixels resampled.
    public static int ResampleDisocclusions(IntPtr converged, IntPtr count, int width, int height, int samples, int bounces,
                                            float below = 1.0f, float weight = 1.0f, float maxHistory = 64.0f) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtTemporal: resample on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        UrtDevice.Check(UrtNative.urt_resample_below(ctx, Wrap(ctx, converged, width, height), Wrap(ctx, count, width, height), below,
                                                     samples, bounces, weight, maxHistory, out int n));
        return n;
    }
}

/// Trace at low resolution, present at full (include/urt.h urt_upsample) over device images the engine owns, all ARGBFloat: the low*
/// images are lowWidth x lowHeight — the accumulated image, optionally its count texture, and the pixel-centre feature buffers
/// UrtFeatureBuffers.Render wrote on the low grid — the others width x height: the same feature buffers on the full grid under the same
/// camera, optionally albedo (the exact sky for sky pixels), and the outputs color and, optionally, count.  A pixel no low-resolution
/// tap can serve gets colour and count 0: UrtTemporal.ResampleDisocclusions(color, count, width, height, ...) with the full-size texture
/// bound as Result fills those.  Refresh both sets of feature buffers whenever the camera or the scene moves, each rendered with
/// _CameraInverseProjection sheared by half a pixel of its grid (include/urt.h "Where the guides should look").  Defaults: include/urt.h
/// URT_UPSAMPLE_DEFAULT_*.
public static class UrtUpscaler {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly Dictionary<IntPtr, ulong> wrappedLow = new Dictionary<IntPtr, ulong>(), wrappedFull = new Dictionary<IntPtr, ulong>();
    static int lw, lh, fw, fh;
    static ulong Wrap(IntPtr ctx, Dictionary<IntPtr, ulong> wrapped, IntPtr p, int width, int height) {
        if (p == IntPtr.Zero) return 0;
        if (!wrapped.TryGetValue(p, out ulong handle)) {
            UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, p, out handle));
            wrapped[p] = handle;
        }
        return handle;
    }
    public static void Upsample(IntPtr lowColor, IntPtr lowHit, IntPtr lowNormal, IntPtr lowId, int lowWidth, int lowHeight,
                                IntPtr hit, IntPtr normal, IntPtr id, IntPtr color, int width, int height,
                                IntPtr count = default(IntPtr), IntPtr lowCount = default(IntPtr), IntPtr albedo = default(IntPtr),
                                float normalThreshold = 0.9f, float planeThreshold = 0.02f, float countScale = 1.0f,
                                bool wideFallback = true, bool skyFromAlbedo = false) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtUpscaler: upsample on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        if (boundCtx != ctx || lw != lowWidth || lh != lowHeight || fw != width || fh != height) {   // re-wrapped when the context or a size changes
            if (boundCtx == ctx) {
                foreach (ulong t in wrappedLow.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
                foreach (ulong t in wrappedFull.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
            }
            wrappedLow.Clear(); wrappedFull.Clear();
            boundCtx = ctx; lw = lowWidth; lh = lowHeight; fw = width; fh = height;
        }
        var im = new UrtNative.UpsampleImages {
            lowColor = Wrap(ctx, wrappedLow, lowColor, lw, lh), lowCount = Wrap(ctx, wrappedLow, lowCount, lw, lh),
            lowHit = Wrap(ctx, wrappedLow, lowHit, lw, lh), lowNormal = Wrap(ctx, wrappedLow, lowNormal, lw, lh), lowId = Wrap(ctx, wrappedLow, lowId, lw, lh),
            hit = Wrap(ctx, wrappedFull, hit, fw, fh), normal = Wrap(ctx, wrappedFull, normal, fw, fh), id = Wrap(ctx, wrappedFull, id, fw, fh),
            albedo = Wrap(ctx, wrappedFull, albedo, fw, fh),
            color = Wrap(ctx, wrappedFull, color, fw, fh), count = Wrap(ctx, wrappedFull, count, fw, fh) };
        var p = new UrtNative.UpsampleParams { normalThreshold = normalThreshold, planeThreshold = planeThreshold, countScale = countScale,
                                               flags = (wideFallback ? UrtNative.UpsampleWideFallback : 0) |
                                                       (skyFromAlbedo ? UrtNative.UpsampleSkyFromAlbedo : 0) };
        UrtDevice.Check(UrtNative.urt_upsample(ctx, in im, in p));
    }
}

/// Auto-exposure and tone mapping (include/urt.h urt_auto_exposure / urt_tonemap) over device images the engine owns, all ARGBFloat of
/// one size: Meter writes the exposure for `src` (RM:12 _converged's RenderTexture; `count` optional, the temporal count texture) into
/// `state`, UrtNative.ExposureStateBytes of 16-byte aligned device memory the host allocated and zero-filled once; ToneMap writes
/// operator(src * exposure) into `dst` (may be src; state IntPtr.Zero = params' exposure alone).  Call both every presented frame, then
/// read `dst` back as RGBA8 sRGB (urt_texture_read_begin_format) in place of the RM:819 blit.  Derive `rate` from the frame time
/// (1 - exp(-dt / tau)); 1 snaps.  Defaults: include/urt.h URT_EXPOSURE_DEFAULT_*, URT_TONEMAP_DEFAULT_*.
public static class UrtToneMapper {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly Dictionary<IntPtr, ulong> wrapped = new Dictionary<IntPtr, ulong>();
    static int w, h;
    static ulong Wrap(IntPtr ctx, IntPtr p, int width, int height) {  // external textures, re-wrapped when the context or the size changes
        if (p == IntPtr.Zero) return 0;
        if (boundCtx != ctx || w != width || h != height) {
            if (boundCtx == ctx) foreach (ulong t in wrapped.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
            wrapped.Clear();
            boundCtx = ctx; w = width; h = height;
        }
        if (!wrapped.TryGetValue(p, out ulong handle)) {
            UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, p, out handle));
            wrapped[p] = handle;
        }
        return handle;
    }
    public static void Meter(IntPtr src, int width, int height, IntPtr state, IntPtr count = default(IntPtr),
                             float key = 0.18f, float minExposure = 0.015625f, float maxExposure = 64.0f, float rate = 1.0f,
                             int lowPermille = 100, int highPermille = 950) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtToneMapper: meter on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var p = new UrtNative.ExposureParams { key = key, minExposure = minExposure, maxExposure = maxExposure, rate = rate,
                                               lowPermille = lowPermille, highPermille = highPermille };
        UrtDevice.Check(UrtNative.urt_auto_exposure(ctx, Wrap(ctx, src, width, height), Wrap(ctx, count, width, height), in p, state));
    }
    public static void ToneMap(IntPtr src, IntPtr dst, int width, int height, IntPtr state = default(IntPtr),
                               int op = UrtNative.TonemapAces, float exposure = 1.0f, float white = 4.0f) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtToneMapper: tone-map on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var p = new UrtNative.TonemapParams { exposure = exposure, white = white, op = op, flags = 0 };
        UrtDevice.Check(UrtNative.urt_tonemap(ctx, Wrap(ctx, src, width, height), Wrap(ctx, dst, width, height), in p, state));
    }
}

/// Bloom (include/urt.h urt_bloom) over device images the engine owns, both ARGBFloat of one size: Apply writes src + intensity * bloom(src)
/// into `dst` (may be src; bloomOnly: the bloom alone).  `state` is the exposure state UrtToneMapper.Meter wrote (IntPtr.Zero: threshold
/// and clamp count in linear radiance).  Per presented frame: UrtToneMapper.Meter(src), UrtBloom.Apply(src, dst), UrtToneMapper.ToneMap(dst,
/// dst), then the RGBA8 sRGB readback of dst.  Defaults: include/urt.h URT_BLOOM_DEFAULT_*.
public static class UrtBloom {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly Dictionary<IntPtr, ulong> wrapped = new Dictionary<IntPtr, ulong>();
    static int w, h;
    static ulong Wrap(IntPtr ctx, IntPtr p, int width, int height) {  // external textures, re-wrapped when the context or the size changes
        if (boundCtx != ctx || w != width || h != height) {
            if (boundCtx == ctx) foreach (ulong t in wrapped.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
            wrapped.Clear();
            boundCtx = ctx; w = width; h = height;
        }
        if (!wrapped.TryGetValue(p, out ulong handle)) {
            UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, p, out handle));
            wrapped[p] = handle;
        }
        return handle;
    }
    public static void Apply(IntPtr src, IntPtr dst, int width, int height, IntPtr state = default(IntPtr),
                             float threshold = 1.0f, float softKnee = 0.5f, float clamp = 65504.0f, float scatter = 0.7f,
                             float intensity = 0.2f, int levels = 6, bool bloomOnly = false) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtBloom: bloom on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var p = new UrtNative.BloomParams { threshold = threshold, softKnee = softKnee, clamp = clamp, scatter = scatter,
                                            intensity = intensity, levels = levels, flags = bloomOnly ? UrtNative.BloomFlagOnly : 0 };
        UrtDevice.Check(UrtNative.urt_bloom(ctx, Wrap(ctx, src, width, height), Wrap(ctx, dst, width, height), in p, state));
    }
}

/// Depth of field (include/urt.h urt_depth_of_field) over device images the engine owns, all ARGBFloat of one size: Apply writes `src`
/// blurred by a thin lens' circle of confusion into `dst` (neither src nor hit).  `hit` is the hit target of urt_render_aov for the
/// same camera: its .w is the distance, +inf for the sky.  Per presented frame: UrtToneMapper.Meter(src), UrtDepthOfField.Apply(src, hit,
/// dst), UrtBloom.Apply(dst, dst), UrtToneMapper.ToneMap(dst, dst), then the RGBA8 sRGB readback of dst.  Scale gives `scale` for a
/// physical camera.  Defaults: include/urt.h URT_DOF_DEFAULT_*.
public static class UrtDepthOfField {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly Dictionary<IntPtr, ulong> wrapped = new Dictionary<IntPtr, ulong>();
    static int w, h;
    static ulong Wrap(IntPtr ctx, IntPtr p, int width, int height) {  // external textures, re-wrapped when the context or the size changes
        if (boundCtx != ctx || w != width || h != height) {
            if (boundCtx == ctx) foreach (ulong t in wrapped.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
            wrapped.Clear();
            boundCtx = ctx; w = width; h = height;
        }
        if (!wrapped.TryGetValue(p, out ulong handle)) {
            UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, p, out handle));
            wrapped[p] = handle;
        }
        return handle;
    }
    /// The blur radius in pixels of a point at infinity: 0.5 * height * f^2 / (N * (s - f) * sensorHeight), lengths in scene units.
    public static float Scale(int height, float focusDistance, float fNumber = 5.6f, float focalLength = 0.05f, float sensorHeight = 0.024f) {
        if (!(focusDistance > focalLength)) throw new ArgumentException("UrtDepthOfField: the focus distance must lie beyond the focal length");
        return (float)(0.5 * height * (double)focalLength * focalLength / ((double)fNumber * ((double)focusDistance - focalLength) * sensorHeight));
    }
    public static void Apply(IntPtr src, IntPtr hit, IntPtr dst, int width, int height,
                             float focusDistance = 10.0f, float scale = 8.0f, float maxRadius = 8.0f, bool showCoc = false) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtDepthOfField: depth of field on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var p = new UrtNative.DofParams { focusDistance = focusDistance, scale = scale, maxRadius = maxRadius,
                                          flags = showCoc ? UrtNative.DofFlagCoc : 0 };
        UrtDevice.Check(UrtNative.urt_depth_of_field(ctx, Wrap(ctx, src, width, height), Wrap(ctx, hit, width, height),
                                                     Wrap(ctx, dst, width, height), in p));
    }
}

/// Motion blur (include/urt.h urt_motion_blur) over device images the engine owns, all ARGBFloat of one size: Apply writes `src`
/// streaked along the motion of the open shutter into `dst` (none of src, motion and hit).  `motion` is the motion image of
/// urt_reproject / urt_reproject_objects / urt_reproject_deformed for the edit the frame shows, `hit` the hit target of urt_render_aov for
/// the same camera.  Per presented frame: UrtToneMapper.Meter(src), UrtDepthOfField.Apply(src, hit, tmp), UrtMotionBlur.Apply(tmp, motion,
/// hit, dst), UrtBloom.Apply(dst, dst), UrtToneMapper.ToneMap(dst, dst), then the RGBA8 sRGB readback of dst.  A frame nothing moved in
/// skips the call.  Defaults: include/urt.h URT_MOTION_BLUR_DEFAULT_*.
public static class UrtMotionBlur {
    static IntPtr boundCtx = IntPtr.Zero;
    static readonly Dictionary<IntPtr, ulong> wrapped = new Dictionary<IntPtr, ulong>();
    static int w, h;
    static ulong Wrap(IntPtr ctx, IntPtr p, int width, int height) {  // external textures, re-wrapped when the context or the size changes
        if (boundCtx != ctx || w != width || h != height) {
            if (boundCtx == ctx) foreach (ulong t in wrapped.Values) UrtDevice.Check(UrtNative.urt_texture_release(ctx, t));
            wrapped.Clear();
            boundCtx = ctx; w = width; h = height;
        }
        if (!wrapped.TryGetValue(p, out ulong handle)) {
            UrtDevice.Check(UrtNative.urt_texture_create_external(ctx, width, height, p, out handle));
            wrapped[p] = handle;
        }
        return handle;
    }
    public static void Apply(IntPtr src, IntPtr motion, IntPtr hit, IntPtr dst, int width, int height,
                             float shutter = 0.5f, float maxRadius = 16.0f, bool showVelocity = false) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtMotionBlur: motion blur on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        var p = new UrtNative.MotionBlurParams { shutter = shutter, maxRadius = maxRadius,
                                                 flags = showVelocity ? UrtNative.MotionBlurFlagVelocity : 0, reserved = 0 };
        UrtDevice.Check(UrtNative.urt_motion_blur(ctx, Wrap(ctx, src, width, height), Wrap(ctx, motion, width, height),
                                                  Wrap(ctx, hit, width, height), Wrap(ctx, dst, width, height), in p));
    }
}

/// new ComputeBuffer(count, stride); .SetData(List<T>); .Release(); .count; .stride            (RM:233-252)
public sealed class UrtComputeBuffer {
    internal ulong handle;
    public int count { get; private set; }
    public int stride { get; private set; }
    public UrtComputeBuffer(int count, int stride) {
        this.count = count; this.stride = stride;
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_buffer_create(UrtDevice.Handle, count, stride, out handle)
                                          : UrtNative.urt_buffer_create(UrtDevice.Handle, count, stride, out handle));
    }
    public void SetData<T>(List<T> data) where T : struct {
        T[] a = data.ToArray();                                   // the library copies before returning (SetData semantics)
        GCHandle pin = GCHandle.Alloc(a, GCHandleType.Pinned);
        try {
            IntPtr p = pin.AddrOfPinnedObject();
            UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_buffer_set_data(UrtDevice.Handle, handle, p, a.Length)
                                              : UrtNative.urt_buffer_set_data(UrtDevice.Handle, handle, p, a.Length));
        } finally { pin.Free(); }
    }
    /// SetData(data, managedBufferStartIndex, computeBufferStartIndex, count): Unity's ranged overload (include/urt.h urt_buffer_set_data_range)
    public void SetData<T>(List<T> data, int managedBufferStartIndex, int computeBufferStartIndex, int count) where T : struct {
        if (managedBufferStartIndex < 0 || count < 0 || managedBufferStartIndex + count > data.Count)
            throw new ArgumentOutOfRangeException(nameof(count), "SetData: the element range lies outside data");
        T[] a = data.GetRange(managedBufferStartIndex, count).ToArray();
        GCHandle pin = GCHandle.Alloc(a, GCHandleType.Pinned);
        try {
            IntPtr p = pin.AddrOfPinnedObject();
            UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_buffer_set_data_range(UrtDevice.Handle, handle, computeBufferStartIndex, p, a.Length)
                                              : UrtNative.urt_buffer_set_data_range(UrtDevice.Handle, handle, computeBufferStartIndex, p, a.Length));
        } finally { pin.Free(); }
    }
    public void Release() {
        if (handle == 0) return;
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_buffer_release(UrtDevice.Handle, handle) : UrtNative.urt_buffer_release(UrtDevice.Handle, handle));
        handle = 0;
    }
}

/// The object-level heaps (_MeshBVH / _SphereBVH) built on the GPU: RayTraceMaster.device_object_heaps of the Python mirror (include/urt.h
/// "the object-level BVH on the device").  For a host whose vertices live on the device (UrtSkinnedMesh) or that does not want the host
/// pass of SetupBVHLeaves / CreateBVH: the boxes are those of the mesh's own points, read from the device side of _Vertices.  It owns the
/// two leaf buffers.  On one context only, as UrtSkinnedMesh.
public sealed class UrtObjectHeaps {
    UrtComputeBuffer meshLeaves, sphereLeaves;
    static UrtComputeBuffer Sized(UrtComputeBuffer b, int count) {
        if (b != null && b.count != count) { b.Release(); b = null; }
        return b ?? new UrtComputeBuffer(count, 28);
    }
    /// Leaf boxes, then the heap, into the device side of meshBvh and sphereBvh (the buffers bound as _MeshBVH / _SphereBVH, sized by
    /// CreateBVH's length for their object counts): five kernels on the context's stream, nothing is waited for; the next frame's
    /// preparation picks the heaps up.  Either triple may be null (no such objects).  More than UrtNative.ObjectBvhDeviceMax objects of one
    /// kind: build that heap on the host.
    public void RebuildObjectHeapsOnDevice(UrtComputeBuffer meshObjects, UrtComputeBuffer vertices, UrtComputeBuffer indices, UrtComputeBuffer meshBvh,
                                           UrtComputeBuffer spheres, UrtComputeBuffer sphereBvh) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtObjectHeaps: build on one rank's context (urt_group_context)");
        IntPtr ctx = UrtDevice.Handle;
        if (meshObjects != null && meshBvh != null) {
            meshLeaves = Sized(meshLeaves, meshObjects.count);
            UrtDevice.Check(UrtNative.urt_mesh_leaf_bounds_device(ctx, meshObjects.handle, vertices.handle, indices.handle, meshLeaves.handle));
            UrtDevice.Check(UrtNative.urt_build_object_bvh_device(ctx, meshLeaves.handle, meshBvh.handle));
        }
        if (spheres != null && sphereBvh != null) {
            sphereLeaves = Sized(sphereLeaves, spheres.count);
            UrtDevice.Check(UrtNative.urt_sphere_leaf_bounds_device(ctx, spheres.handle, sphereLeaves.handle));
            UrtDevice.Check(UrtNative.urt_build_object_bvh_device(ctx, sphereLeaves.handle, sphereBvh.handle));
        }
    }
    public void Release() {
        if (meshLeaves != null) { meshLeaves.Release(); meshLeaves = null; }
        if (sphereLeaves != null) { sphereLeaves.Release(); sphereLeaves = null; }
    }
}

/// Geometry that is made on the GPU (an LOD switch, procedural or re-meshed geometry): RayTraceMaster.ReplaceGeometryDevice and
/// device_prepare of the Python mirror (include/urt.h "the device side of a ComputeBuffer", option "prepare_device").  It owns the three
/// geometry buffers a host binds as _Vertices / _Indices / _Normals; with DevicePrepare on, the full preparation that new topology asks
/// for reads them where they are: nothing is downloaded, and the triangle BVHs are built on the GPU.  On one context only, as UrtSkinnedMesh.
public sealed class UrtDeviceGeometry {
    public UrtComputeBuffer vertices, indices, normals;
    /// Option "prepare_device" of the context (off by default: a full preparation downloads device-written geometry first).
    public static void SetDevicePrepare(bool on) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtDeviceGeometry: set the option on one rank's context (urt_group_context)");
        UrtDevice.Check(UrtNative.urt_set_option(UrtDevice.Handle, "prepare_device", on ? 1 : 0));
    }
    static UrtComputeBuffer FromDevice(UrtComputeBuffer b, IntPtr deviceData, int count, int stride) {
        if (b != null && b.count != count) { b.Release(); b = null; }                 // a buffer whose count fits is reused
        if (b == null) b = new UrtComputeBuffer(count, stride);                       // else a new one, with this write as its first and only
        UrtDevice.Check(UrtNative.urt_buffer_set_data_device(UrtDevice.Handle, b.handle, 0, deviceData, count));
        return b;
    }
    /// The three lists from device memory (4-byte aligned addresses, element counts; the copies are enqueued on the context's stream and
    /// the caller orders their producers).  The caller then binds the buffers, sets _MeshObjects through SetData, supplies _MeshBVH
    /// (UrtObjectHeaps.RebuildObjectHeapsOnDevice builds it without a host pass) and restarts its accumulation: topology changed, so no
    /// history is kept.
    public void ReplaceGeometryDevice(IntPtr deviceVertices, int nVertices, IntPtr deviceIndices, int nIndices, IntPtr deviceNormals, int nNormals) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtDeviceGeometry: replace on one rank's context (urt_group_context)");
        vertices = FromDevice(vertices, deviceVertices, nVertices, 12);
        indices = FromDevice(indices, deviceIndices, nIndices, 4);
        normals = FromDevice(normals, deviceNormals, nNormals, 12);
    }
    public void Release() {
        if (vertices != null) { vertices.Release(); vertices = null; }
        if (indices != null) { indices.Release(); indices = null; }
        if (normals != null) { normals.Release(); normals = null; }
    }
}

/// A skinned mesh animated on the GPU: RayTraceMaster.AttachSkin / SkinMeshes of the Python mirror (include/urt.h urt_skin_vertices,
/// urt_buffer_bounds).  One instance serves every skinned MeshObject of a scene: it owns rest-pose, bone-index and bone-weight buffers of
/// the vertex count and one bone table per mesh.  Per frame only the bones travel; the positions are written into the device side of the
/// _Vertices / _Normals buffers and the library refits the skinned meshes in place (option "refit_vertices").  On one context only: a
/// group host reaches the ranks through urt_group_context.
public sealed class UrtSkinnedMesh {
    sealed class Skin { public int first, count; public ulong bones; public int nBones; public bool morphed; }   // morphed: MorphMesh(intoRestPose) has written this frame's rest pose
    readonly UrtComputeBuffer restVertices, restNormals, boneIndices, boneWeights;
    readonly Dictionary<int, Skin> skins = new Dictionary<int, Skin>();
    public UrtSkinnedMesh(int vertexCount) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtSkinnedMesh: skin on one rank's context (urt_group_context)");
        restVertices = new UrtComputeBuffer(vertexCount, 12); restNormals = new UrtComputeBuffer(vertexCount, 12);
        boneIndices = new UrtComputeBuffer(vertexCount, 16); boneWeights = new UrtComputeBuffer(vertexCount, 16);
    }
    /// The vertex span first .. first + count - 1 of MeshObject meshIndex gets a skin: its rest pose (mesh.vertices / mesh.normals) and per
    /// vertex four bone indices (BoneWeight.boneIndex0..3) and weights (BoneWeight.weight0..3), four ints / floats per vertex.
    public void AttachSkin(int meshIndex, int first, List<Vector3> restPositions, List<Vector3> restNormalList, List<int> indices4, List<float> weights4) {
        int count = restPositions.Count;
        if (restNormalList.Count != count || indices4.Count != 4 * count || weights4.Count != 4 * count)
            throw new ArgumentException("UrtSkinnedMesh.AttachSkin: the lists do not describe one vertex span");
        restVertices.SetData(restPositions, 0, first, count);
        restNormals.SetData(restNormalList, 0, first, count);
        SetWords(boneIndices, indices4.ToArray(), first, count);
        SetWords(boneWeights, weights4.ToArray(), first, count);
        skins[meshIndex] = new Skin { first = first, count = count };
    }
    static void SetWords<T>(UrtComputeBuffer b, T[] words, int first, int count) where T : struct {
        GCHandle pin = GCHandle.Alloc(words, GCHandleType.Pinned);
        try { UrtDevice.Check(UrtNative.urt_buffer_set_data_range(UrtDevice.Handle, b.handle, first, pin.AddrOfPinnedObject(), count)); }
        finally { pin.Free(); }
    }
    /// poses: MeshObject index -> its bones, 12 floats each (three columns of the linear part, then the translation), from the mesh's object
    /// space to itself: worldToLocal(mesh) * SkinnedMeshRenderer.bones[i].localToWorldMatrix * sharedMesh.bindposes[i].  Skins every span
    /// into `vertices` / `normals` (the buffers bound as _Vertices / _Normals) and returns, per mesh, the object-space bounds of its
    /// skinned vertices (min.xyz, max.xyz) as the GPU found them: the caller transforms the eight corners by localToWorldMatrix for the
    /// mesh's _MeshBVH leaf box (RM:405-433), rebuilds the heap and SetData-s it, as after any deformation.
    public Dictionary<int, float[]> SkinMeshes(Dictionary<int, float[]> poses, UrtComputeBuffer vertices, UrtComputeBuffer normals) {
        IntPtr ctx = UrtDevice.Handle;
        foreach (var kv in poses) {
            if (!skins.TryGetValue(kv.Key, out Skin s)) throw new ArgumentException("UrtSkinnedMesh.SkinMeshes: MeshObject " + kv.Key + " has no skin (AttachSkin)");
            int nBones = kv.Value.Length / 12;
            if (nBones < 1 || kv.Value.Length != 12 * nBones) throw new ArgumentException("UrtSkinnedMesh.SkinMeshes: 12 floats per bone");
            if (s.bones != 0 && s.nBones != nBones) { UrtDevice.Check(UrtNative.urt_buffer_release(ctx, s.bones)); s.bones = 0; }
            if (s.bones == 0) UrtDevice.Check(UrtNative.urt_buffer_create(ctx, nBones, UrtNative.ObjectMotionStride, out s.bones));
            s.nBones = nBones;
            GCHandle pin = GCHandle.Alloc(kv.Value, GCHandleType.Pinned);
            try { UrtDevice.Check(UrtNative.urt_buffer_set_data(ctx, s.bones, pin.AddrOfPinnedObject(), nBones)); }
            finally { pin.Free(); }
            UrtComputeBuffer rv = s.morphed ? morphedVertices : restVertices, rn = s.morphed ? morphedNormals : restNormals;   // blend shapes come before the bones
            s.morphed = false;
            var sb = new UrtNative.SkinBuffers { restVertices = rv.handle, restNormals = normals != null ? rn.handle : 0,
                                                 boneIndices = boneIndices.handle, boneWeights = boneWeights.handle, bones = s.bones };
            UrtDevice.Check(UrtNative.urt_skin_vertices(ctx, in sb, s.first, s.count, vertices.handle, normals != null ? normals.handle : 0));
        }
        var boxes = new Dictionary<int, float[]>();
        foreach (var kv in poses) {                                   // after every kernel is enqueued: each bounds call waits
            Skin s = skins[kv.Key];
            var box = new float[6];
            UrtDevice.Check(UrtNative.urt_buffer_bounds(ctx, vertices.handle, s.first, s.count, box, out int _));
            boxes[kv.Key] = box;
        }
        return boxes;
    }
    // ---- blend shapes (include/urt.h urt_morph_vertices): the stage of a SkinnedMeshRenderer that comes before the bones ----
    sealed class Morph { public int first, count, nTargets; public ulong plan, weights; public float[] frameWeights; }
    readonly Dictionary<int, Morph> morphs = new Dictionary<int, Morph>();
    UrtComputeBuffer morphedVertices, morphedNormals;                 // what a morph ahead of a skin writes and the skin reads: device side only
    /// The vertex span of MeshObject meshIndex (the one AttachSkin named, or `first` on) gets the blend shapes of renderer.sharedMesh:
    /// sharedMesh.blendShapeCount targets, each the LAST frame of its shape (GetBlendShapeFrameVertices of frame
    /// GetBlendShapeFrameCount - 1), whose weight is GetBlendShapeWeight / GetBlendShapeFrameWeight of that frame.  In-between frames
    /// are out of scope: a shape with several frames is blended linearly from the rest pose to its last frame.  Rows whose six deltas are
    /// all zero are dropped.  The rest pose is the one AttachSkin uploaded, or mesh.vertices / mesh.normals for a mesh without a skin.
    public void AttachBlendShapes(int meshIndex, int first, SkinnedMeshRenderer renderer) {
        Mesh mesh = renderer.sharedMesh;
        int count = mesh.vertexCount, nTargets = mesh.blendShapeCount;
        if (nTargets < 1) throw new ArgumentException("UrtSkinnedMesh.AttachBlendShapes: the mesh has no blend shapes");
        if (!skins.ContainsKey(meshIndex)) {
            restVertices.SetData(new List<Vector3>(mesh.vertices), 0, first, count);
            restNormals.SetData(new List<Vector3>(mesh.normals), 0, first, count);
        }
        var deltas = new List<UrtNative.MorphDelta>();
        var frameWeights = new float[nTargets];
        Vector3[] dp = new Vector3[count], dn = new Vector3[count], dt = new Vector3[count];
        for (int t = 0; t < nTargets; t++) {
            int last = mesh.GetBlendShapeFrameCount(t) - 1;
            frameWeights[t] = mesh.GetBlendShapeFrameWeight(t, last);
            mesh.GetBlendShapeFrameVertices(t, last, dp, dn, dt);    // (tangents are not carried)
            for (int v = 0; v < count; v++)
                if (dp[v].x != 0f || dp[v].y != 0f || dp[v].z != 0f || dn[v].x != 0f || dn[v].y != 0f || dn[v].z != 0f)   // (component by component: Vector3's == is approximate)
                    deltas.Add(new UrtNative.MorphDelta { vertex = first + v, target = t, dpx = dp[v].x, dpy = dp[v].y, dpz = dp[v].z,
                                                          dnx = dn[v].x, dny = dn[v].y, dnz = dn[v].z });
        }
        if (morphs.TryGetValue(meshIndex, out Morph old)) ReleaseMorph(old);
        var m = new Morph { first = first, count = count, nTargets = nTargets, frameWeights = frameWeights };
        UrtDevice.Check(UrtNative.urt_morph_plan_create(UrtDevice.Handle, deltas.ToArray(), deltas.Count, nTargets, first, count, out m.plan));
        UrtDevice.Check(UrtNative.urt_buffer_create(UrtDevice.Handle, nTargets, 4, out m.weights));
        morphs[meshIndex] = m;
    }
    /// Uploads renderer.GetBlendShapeWeight(t) / frameWeight(t) for every target and morphs the span.  Ahead of SkinMeshes (intoRestPose):
    /// into a pair of intermediate buffers that SkinMeshes then takes as this mesh's rest pose, so blend shapes come before the bones and
    /// the morphed rest pose never crosses the bus.  Else straight into `vertices` / `normals` (normals normalised); then the caller owes
    /// the bounds and the heap as after SkinMeshes (urt_buffer_bounds).
    public void MorphMesh(int meshIndex, SkinnedMeshRenderer renderer, bool intoRestPose, UrtComputeBuffer vertices, UrtComputeBuffer normals) {
        if (!morphs.TryGetValue(meshIndex, out Morph m)) throw new ArgumentException("UrtSkinnedMesh.MorphMesh: MeshObject " + meshIndex + " has no blend shapes (AttachBlendShapes)");
        var w = new float[m.nTargets];
        for (int t = 0; t < m.nTargets; t++) w[t] = renderer.GetBlendShapeWeight(t) / m.frameWeights[t];
        GCHandle pin = GCHandle.Alloc(w, GCHandleType.Pinned);
        try { UrtDevice.Check(UrtNative.urt_buffer_set_data(UrtDevice.Handle, m.weights, pin.AddrOfPinnedObject(), m.nTargets)); }
        finally { pin.Free(); }
        if (intoRestPose) {
            if (morphedVertices == null) { morphedVertices = new UrtComputeBuffer(restVertices.count, 12); morphedNormals = new UrtComputeBuffer(restVertices.count, 12); }
            UrtDevice.Check(UrtNative.urt_morph_vertices(UrtDevice.Handle, m.plan, restVertices.handle, restNormals.handle, m.weights,
                                                         morphedVertices.handle, morphedNormals.handle, 0));
            if (skins.TryGetValue(meshIndex, out Skin s)) s.morphed = true;
        } else {
            UrtDevice.Check(UrtNative.urt_morph_vertices(UrtDevice.Handle, m.plan, restVertices.handle, normals != null ? restNormals.handle : 0, m.weights,
                                                         vertices.handle, normals != null ? normals.handle : 0, normals != null ? UrtNative.MorphNormalize : 0));
        }
    }
    void ReleaseMorph(Morph m) {
        if (m.plan != 0) { UrtDevice.Check(UrtNative.urt_morph_plan_release(UrtDevice.Handle, m.plan)); m.plan = 0; }
        if (m.weights != 0) { UrtDevice.Check(UrtNative.urt_buffer_release(UrtDevice.Handle, m.weights)); m.weights = 0; }
    }
    public void Release() {
        foreach (var s in skins.Values) if (s.bones != 0) { UrtDevice.Check(UrtNative.urt_buffer_release(UrtDevice.Handle, s.bones)); s.bones = 0; }
        foreach (var m in morphs.Values) ReleaseMorph(m);
        if (morphedVertices != null) { morphedVertices.Release(); morphedNormals.Release(); morphedVertices = morphedNormals = null; }
        restVertices.Release(); restNormals.Release(); boneIndices.Release(); boneWeights.Release();
    }
}

/// RayTraceMaster.ComputeNormals (RM:340-368) on the GPU for a vertex span whose positions were written on the device (UrtSkinnedMesh, a
/// SetData from device memory): include/urt.h urt_normals_plan_create / urt_compute_normals.  The plan is made once per topology from the
/// buffers as they are then (a synchronising set-up call); Compute enqueues two kernels that write the span's normals into the device
/// side of the _Normals buffer, where the in-place update picks them up.  A host that changes _Indices, or whose deformation merges or
/// splits coincident vertices, makes a new plan.  On one context only, as UrtSkinnedMesh.
public sealed class UrtNormalsPlan {
    ulong handle;
    public UrtNormalsPlan(UrtComputeBuffer vertices, UrtComputeBuffer indices, int first, int count) {
        if (UrtDevice.IsGroup) throw new InvalidOperationException("UrtNormalsPlan: plan on one rank's context (urt_group_context)");
        UrtDevice.Check(UrtNative.urt_normals_plan_create(UrtDevice.Handle, vertices.handle, indices.handle, first, count, out handle));
    }
    /// served vertices, welded lists, needed triangles, contributing slots, the longest list, bytes on the device
    public void Info(out int first, out int count, out int lists, out int triangles, out int entries, out int maxValence, out ulong deviceBytes) {
        UrtDevice.Check(UrtNative.urt_normals_plan_info(UrtDevice.Handle, handle, out UrtNative.NormalsPlanInfo i));
        first = i.first; count = i.count; lists = i.nLists; triangles = i.nTriangles; entries = i.nEntries; maxValence = i.maxValence; deviceBytes = i.deviceBytes;
    }
    public void Compute(UrtComputeBuffer dstNormals) { UrtDevice.Check(UrtNative.urt_compute_normals(UrtDevice.Handle, handle, dstNormals.handle)); }
    public void Release() { if (handle != 0) { UrtDevice.Check(UrtNative.urt_normals_plan_release(UrtDevice.Handle, handle)); handle = 0; } }
}

/// new RenderTexture(w, h, 0, ARGBFloat, Linear) { enableRandomWrite = true }.Create(); .Release(); .width; .height   (RM:824-845)
public sealed class UrtRenderTexture {
    internal ulong handle;
    public int width { get; private set; }
    public int height { get; private set; }
    public bool enableRandomWrite;                                  // accepted: every image here is writable
    public UrtRenderTexture(int width, int height, int depth, RenderTextureFormat format, RenderTextureReadWrite readWrite) {
        this.width = width; this.height = height;                   // format is ARGBFloat / Linear at the only call site (RM:834-840)
    }
    public bool Create() {
        if (handle != 0) return true;
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_texture_create(UrtDevice.Handle, width, height, out handle)
                                          : UrtNative.urt_texture_create(UrtDevice.Handle, width, height, out handle));
        return handle != 0;
    }
    public void Release() {
        if (handle == 0) return;
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_texture_release(UrtDevice.Handle, handle) : UrtNative.urt_texture_release(UrtDevice.Handle, handle));
        handle = 0;
    }
    /// Upload RGBA32F texels, row 0 = bottom (Unity's own row order): the sky (RM:776) after Texture2D.GetPixelData<float>.
    public void SetPixels(float[] rgba) {
        Create();
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_texture_set_pixels(UrtDevice.Handle, handle, rgba) : UrtNative.urt_texture_set_pixels(UrtDevice.Handle, handle, rgba));
    }
    public void GetPixels(float[] rgba) {
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_texture_get_pixels(UrtDevice.Handle, handle, rgba) : UrtNative.urt_texture_get_pixels(UrtDevice.Handle, handle, rgba));
    }
}

/// RayTraceShader.SetMatrix/SetVector/SetFloat/SetInt/SetTexture/SetBuffer/Dispatch                (RM:255-259, 772-810)
public sealed class UrtComputeShader {
    public int FindKernel(string name) { return 0; }                // CSMain
    public void SetMatrix(string name, Matrix4x4 m) { UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_set_matrix(UrtDevice.Handle, name, ref m) : UrtNative.urt_shader_set_matrix(UrtDevice.Handle, name, ref m)); }
    public void SetVector(string name, Vector4 v) { UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_set_vector(UrtDevice.Handle, name, ref v) : UrtNative.urt_shader_set_vector(UrtDevice.Handle, name, ref v)); }
    public void SetFloat(string name, float v) { UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_set_float(UrtDevice.Handle, name, v) : UrtNative.urt_shader_set_float(UrtDevice.Handle, name, v)); }
    public void SetInt(string name, int v) { UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_set_int(UrtDevice.Handle, name, v) : UrtNative.urt_shader_set_int(UrtDevice.Handle, name, v)); }
    public void SetTexture(int kernel, string name, UrtRenderTexture t) {
        ulong h = t == null ? 0 : t.handle;
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_set_texture(UrtDevice.Handle, kernel, name, h) : UrtNative.urt_shader_set_texture(UrtDevice.Handle, kernel, name, h));
    }
    public void SetBuffer(int kernel, string name, UrtComputeBuffer b) {
        ulong h = b == null ? 0 : b.handle;
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_set_buffer(UrtDevice.Handle, kernel, name, h) : UrtNative.urt_shader_set_buffer(UrtDevice.Handle, kernel, name, h));
    }
    /// On a group the dispatch is partitioned: rank r traces the 8-row strips r, r+N, ... (same pixels as one full dispatch).
    public void Dispatch(int kernel, int gx, int gy, int gz) {
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_shader_dispatch(UrtDevice.Handle, kernel, gx, gy, gz) : UrtNative.urt_shader_dispatch(UrtDevice.Handle, kernel, gx, gy, gz));
    }
}

/// _additionMaterial.SetFloat("_Sample", n) + Graphics.Blit(src, dst, _additionMaterial); Graphics.Blit(src, dst)   (RM:813-819)
public sealed class UrtAdditionMaterial {
    float sample;
    public void SetFloat(string name, float v) { if (name == "_Sample") sample = v; }
    internal float Sample { get { return sample; } }
}

public static class UrtGraphics {
    public static void Blit(UrtRenderTexture src, UrtRenderTexture dst, UrtAdditionMaterial mat) {       // RM:818
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_blit_add(UrtDevice.Handle, src.handle, dst.handle, mat.Sample)
                                          : UrtNative.urt_blit_add(UrtDevice.Handle, src.handle, dst.handle, mat.Sample));
    }
    /// RM:819 "present": on one device a copy — queued behind the deferred frames and fused into the blend pass, so presenting every
    /// frame keeps the 64-frame launches (include/urt.h "Frame batching"); on a group THE frame-end gather — every rank's strips of
    /// `src` -> the full image `dst` on rank 0.
    public static void Blit(UrtRenderTexture src, UrtRenderTexture dst) {
        UrtDevice.Check(UrtDevice.IsGroup ? UrtNative.urt_group_gather(UrtDevice.Handle, src.handle, dst.handle)
                                          : UrtNative.urt_blit(UrtDevice.Handle, src.handle, dst.handle));
    }
    /// Present through Unity WITHOUT stalling the tracer: the frame that is presented is the previous call's (one frame of latency).
    /// urt_texture_read_begin snapshots `src` and sends it to a pinned host image on a copy stream while the next frames render;
    /// urt_texture_read_end hands that image out, and Texture2D.LoadRawTextureData takes it without a managed copy.
    static ulong pendingTicket = 0;
    public static void BlitPipelined(UrtRenderTexture src, RenderTexture unityDestination, ref Texture2D staging) {
        if (UrtDevice.IsGroup) throw new NotSupportedException("pipelined readback is per device: gather to rank 0's image first");
        // The image crosses the bus in the destination's OWN format, converted on the GPU (csrc/present.hip): an 8-bit back buffer of this
        // linear-colour-space project gets sRGB-encoded bytes (8.3 MB per 1080p frame instead of 33.2 MB), an HDR camera's ARGBHalf halfs.
        bool hdr = unityDestination != null && unityDestination.format == RenderTextureFormat.ARGBHalf;
        TextureFormat tf = hdr ? TextureFormat.RGBAHalf : TextureFormat.RGBA32;
        if (staging == null || staging.width != src.width || staging.height != src.height || staging.format != tf)
            staging = new Texture2D(src.width, src.height, tf, false, /* linear: */ hdr);   // RGBA32 declared sRGB: sampling decodes, the blit re-encodes
        if (pendingTicket != 0) {
            IntPtr pixels; UIntPtr bytes;
            UrtDevice.Check(UrtNative.urt_texture_read_end_format(UrtDevice.Handle, pendingTicket, out pixels, out bytes));
            staging.LoadRawTextureData(pixels, (int)bytes.ToUInt32());
            staging.Apply(false);
            Graphics.Blit(staging, unityDestination);
        }
        UrtDevice.Check(UrtNative.urt_texture_read_begin_format(UrtDevice.Handle, src.handle,
                                                                hdr ? UrtNative.URT_FORMAT_RGBA16F : UrtNative.URT_FORMAT_RGBA8_SRGB, out pendingTicket));
    }
    /// Present through Unity: read the image back (this submits and waits) and hand it to a Unity RenderTexture.
    public static void Blit(UrtRenderTexture src, RenderTexture unityDestination, ref Texture2D staging, ref float[] managed) {
        int n = src.width * src.height * 4;
        if (managed == null || managed.Length != n) managed = new float[n];
        src.GetPixels(managed);
        if (staging == null || staging.width != src.width || staging.height != src.height)
            staging = new Texture2D(src.width, src.height, TextureFormat.RGBAFloat, false, true);
        staging.SetPixelData(managed, 0);
        staging.Apply(false);
        Graphics.Blit(staging, unityDestination);
    }
}
