// UrtNative.cs — P/Invoke declarations for libunityraytracer_amd.so (include/urt.h, ABI version 4; a negative urt_abi_version() = an experiment build: refuse it).
// Drop into Assets/Scripts/ of RemyMuj/UnityRayTracer next to RayTraceMaster.cs ("RM"); the native library goes to
// Assets/Plugins/x86_64/libunityraytracer_amd.so.  One declaration per exported entry point, in the header's order; each
// group cites the RM call site it stands in for.  SOURCE ONLY: the build image of this repository has no C#/.NET/Mono
// toolchain, so this file has not been compiled there; the same ABI is exercised by unityraytracer_amd/_lib.py (ctypes).
using System;
using System.Runtime.InteropServices;

internal static class UrtNative {
    const string Lib = "unityraytracer_amd";

    // ---- library / context ------------------------------------------------------------------------------------------
    [DllImport(Lib)] internal static extern int urt_abi_version();
    [DllImport(Lib)] internal static extern int urt_device_count(out int count);
    [DllImport(Lib)] internal static extern int urt_context_create(int device, out IntPtr ctx);
    [DllImport(Lib)] internal static extern int urt_context_destroy(IntPtr ctx);
    [DllImport(Lib)] internal static extern IntPtr urt_last_error(IntPtr ctx);                      // const char*, never NULL
    [DllImport(Lib)] internal static extern int urt_context_set_stream(IntPtr ctx, IntPtr hipStream);
    [DllImport(Lib)] internal static extern int urt_synchronize(IntPtr ctx);
    [DllImport(Lib)] internal static extern int urt_flush(IntPtr ctx);                              // submit batched frames, no wait

    // ---- ComputeBuffer                                                                     RM:233-252, 195-210 --------
    [DllImport(Lib)] internal static extern int urt_buffer_create(IntPtr ctx, int count, int stride, out ulong buffer);
    [DllImport(Lib)] internal static extern int urt_buffer_set_data(IntPtr ctx, ulong buffer, IntPtr data, int count);
    [DllImport(Lib)] internal static extern int urt_buffer_set_data_range(IntPtr ctx, ulong buffer, int first, IntPtr data, int count);
    // the device side of a buffer (include/urt.h): SetData from device memory, GetData, skinning, bounds, where the contents live
    [StructLayout(LayoutKind.Sequential)] internal struct SkinBuffers { public ulong restVertices, restNormals, boneIndices, boneWeights, bones; }   // 40 B; restNormals 0 = positions only
    [DllImport(Lib)] internal static extern int urt_buffer_set_data_device(IntPtr ctx, ulong buffer, int first, IntPtr deviceData, int count);
    [DllImport(Lib)] internal static extern int urt_buffer_get_data_range(IntPtr ctx, ulong buffer, int first, IntPtr outData, int count);
    [DllImport(Lib)] internal static extern int urt_skin_vertices(IntPtr ctx, in SkinBuffers buffers, int first, int count, ulong dstVertices, ulong dstNormals);
    [DllImport(Lib)] internal static extern int urt_buffer_bounds(IntPtr ctx, ulong buffer, int first, int count, [Out] float[] out6, out int finiteElements);
    [DllImport(Lib)] internal static extern int urt_debug_buffer_state(IntPtr ctx, ulong buffer, [Out] ulong[] out4);   // stale first, stale last, mirror bytes, downloads
    // normals on the device (include/urt.h): ComputeNormals of positions that live in a buffer's device mirror, over a plan made once per topology
    [StructLayout(LayoutKind.Sequential)] internal struct NormalsPlanInfo { public int first, count, nLists, nTriangles, nEntries, maxValence; public ulong deviceBytes; }   // 32 B
    [DllImport(Lib)] internal static extern int urt_normals_plan_create(IntPtr ctx, ulong vertices, ulong indices, int first, int count, out ulong plan);
    [DllImport(Lib)] internal static extern int urt_normals_plan_info(IntPtr ctx, ulong plan, out NormalsPlanInfo info);
    [DllImport(Lib)] internal static extern int urt_normals_plan_release(IntPtr ctx, ulong plan);
    [DllImport(Lib)] internal static extern int urt_compute_normals(IntPtr ctx, ulong plan, ulong dstNormals);
    [DllImport(Lib)] internal static extern int urt_debug_build_normals_plan(float[] vertices, int nVertices, int[] indices, int nIndices, int first, int count, [Out] int[] ranges, [Out] int[] entries, int capEntries, [Out] int[] tris, int capTris, [Out] int[] outSizes3);
    // blend shapes on the device (include/urt.h): per-target vertex deltas added to the rest pose under a weight table, ahead of the bones
    [StructLayout(LayoutKind.Sequential)] internal struct MorphDelta { public int vertex, target; public float dpx, dpy, dpz, dnx, dny, dnz; }   // 32 B; vertex is absolute
    [StructLayout(LayoutKind.Sequential)] internal struct MorphPlanInfo { public int first, count, nTargets, nEntries, maxValence, nTouched; public ulong deviceBytes; }   // 32 B
    internal const int MorphNormalize = 1;   // URT_MORPH_NORMALIZE
    [DllImport(Lib)] internal static extern int urt_morph_plan_create(IntPtr ctx, MorphDelta[] deltas, int nDeltas, int nTargets, int first, int count, out ulong plan);
    [DllImport(Lib)] internal static extern int urt_morph_plan_info(IntPtr ctx, ulong plan, out MorphPlanInfo info);
    [DllImport(Lib)] internal static extern int urt_morph_plan_release(IntPtr ctx, ulong plan);
    [DllImport(Lib)] internal static extern int urt_morph_vertices(IntPtr ctx, ulong plan, ulong restVertices, ulong restNormals, ulong weights, ulong dstVertices, ulong dstNormals, int flags);
    [DllImport(Lib)] internal static extern int urt_debug_build_morph_plan(MorphDelta[] deltas, int nDeltas, int nTargets, int first, int count, [Out] int[] ranges, [Out] int[] order, [Out] int[] outSizes3);
    // the object-level BVH on the device (include/urt.h): leaf boxes and the implicit heap written into the device side of buffers; nothing is waited for
    internal const int ObjectBvhDeviceMax = 1024;   // URT_OBJECT_BVH_DEVICE_MAX
    [DllImport(Lib)] internal static extern int urt_mesh_leaf_bounds_device(IntPtr ctx, ulong meshObjects, ulong vertices, ulong indices, ulong dstLeaves);
    [DllImport(Lib)] internal static extern int urt_sphere_leaf_bounds_device(IntPtr ctx, ulong spheres, ulong dstLeaves);
    [DllImport(Lib)] internal static extern int urt_build_object_bvh_device(IntPtr ctx, ulong leaves, ulong dstNodes);
    [DllImport(Lib)] internal static extern int urt_buffer_get_info(IntPtr ctx, ulong buffer, out int count, out int stride);
    [DllImport(Lib)] internal static extern int urt_buffer_release(IntPtr ctx, ulong buffer);

    // ---- RenderTexture / Texture (ARGBFloat, linear)                                        RM:824-845 -----------------
    [DllImport(Lib)] internal static extern int urt_texture_create(IntPtr ctx, int width, int height, out ulong texture);
    [DllImport(Lib)] internal static extern int urt_texture_create_external(IntPtr ctx, int width, int height, IntPtr devicePtr, out ulong texture);
    [DllImport(Lib)] internal static extern int urt_texture_set_pixels(IntPtr ctx, ulong texture, float[] rgba);
    [DllImport(Lib)] internal static extern int urt_texture_get_pixels(IntPtr ctx, ulong texture, [Out] float[] rgba);
    [DllImport(Lib)] internal static extern int urt_texture_get_info(IntPtr ctx, ulong texture, out int width, out int height, out IntPtr devicePtr);
    [DllImport(Lib)] internal static extern int urt_texture_release(IntPtr ctx, ulong texture);

    // ---- ComputeShader (kernel 0 = CSMain)                                                  RM:772-810 -----------------
    [DllImport(Lib)] internal static extern int urt_shader_set_buffer(IntPtr ctx, int kernel, string name, ulong buffer);
    [DllImport(Lib)] internal static extern int urt_shader_set_texture(IntPtr ctx, int kernel, string name, ulong texture);
    [DllImport(Lib)] internal static extern int urt_shader_set_matrix(IntPtr ctx, string name, ref UnityEngine.Matrix4x4 m);
    [DllImport(Lib)] internal static extern int urt_shader_set_vector(IntPtr ctx, string name, ref UnityEngine.Vector4 v);
    [DllImport(Lib)] internal static extern int urt_shader_set_float(IntPtr ctx, string name, float v);
    [DllImport(Lib)] internal static extern int urt_shader_set_int(IntPtr ctx, string name, int v);
    [DllImport(Lib)] internal static extern int urt_shader_dispatch(IntPtr ctx, int kernel, int gx, int gy, int gz);
    // multi-GPU form of Dispatch: only the 8-row strips firstGroupRow, +rowStride, ... (global pixel ids kept)
    [DllImport(Lib)] internal static extern int urt_shader_dispatch_rows(IntPtr ctx, int kernel, int gx, int gy, int gz, int firstGroupRow, int rowStride);

    // ---- Graphics.Blit                                                                      RM:817-819 -----------------
    [DllImport(Lib)] internal static extern int urt_blit_add(IntPtr ctx, ulong src, ulong dst, float sample);
    [DllImport(Lib)] internal static extern int urt_blit(IntPtr ctx, ulong src, ulong dst);
    // strips <-> dense device buffer for the frame-end gather of a one-process-per-GPU host
    [DllImport(Lib)] internal static extern int urt_texture_pack_rows(IntPtr ctx, ulong texture, int firstGroupRow, int rowStride, IntPtr deviceDst, out ulong bytes);
    [DllImport(Lib)] internal static extern int urt_texture_unpack_rows(IntPtr ctx, ulong texture, int firstGroupRow, int rowStride, IntPtr deviceSrc);
    [DllImport(Lib)] internal static extern int urt_texture_unpack_rows_on(IntPtr ctx, ulong texture, int firstGroupRow, int rowStride, IntPtr deviceSrc, IntPtr hipStream);
    [DllImport(Lib)] internal static extern int urt_texture_read_begin(IntPtr ctx, ulong texture, out ulong ticket);
    [DllImport(Lib)] internal static extern int urt_texture_read_end(IntPtr ctx, ulong ticket, out IntPtr rgba);   // pinned host image, width x height x 4 floats
    internal const int URT_FORMAT_RGBA32F = 0, URT_FORMAT_RGBA8_SRGB = 1, URT_FORMAT_RGBA16F = 2;
    [DllImport(Lib)] internal static extern int urt_texture_read_begin_format(IntPtr ctx, ulong texture, int format, out ulong ticket);   // converted on the GPU to the destination's format
    [DllImport(Lib)] internal static extern int urt_texture_read_end_format(IntPtr ctx, ulong ticket, out IntPtr pixels, out UIntPtr bytes);
    [DllImport(Lib)] internal static extern int urt_texture_pack_rows_rgb(IntPtr ctx, ulong texture, int firstGroupRow, int rowStride, IntPtr deviceDst, out ulong bytes);
    [DllImport(Lib)] internal static extern int urt_texture_unpack_rows_rgb(IntPtr ctx, ulong texture, int firstGroupRow, int rowStride, IntPtr deviceSrc, float alpha, IntPtr hipStream);

    // ---- ray queries (include/urt.h "ray queries"; records of include/urt_types.h) -------------------------------------
    [StructLayout(LayoutKind.Sequential, Pack = 1)]
    internal struct Ray {                                   // urt_Ray, 32 B
        public float ox, oy, oz, tMax;
        public float dx, dy, dz;
        public int reserved;
    }
    [StructLayout(LayoutKind.Sequential, Pack = 1)]
    internal struct RayHit {                                // urt_RayHit, 48 B
        public float distance, px, py, pz, nx, ny, nz;
        public int kind, obj, primitive;                    // kind: 0 miss, 1 ground plane, 2 sphere, 3 triangle
        public float u, v;
    }
    internal const int QueryClosest = 0, QueryAny = 1;
    [DllImport(Lib)] internal static extern int urt_ray_query(IntPtr ctx, [In] Ray[] rays, int n, [Out] RayHit[] hits, int flags);
    [DllImport(Lib, EntryPoint = "urt_ray_query")] internal static extern int urt_ray_query_any(IntPtr ctx, [In] Ray[] rays, int n, [Out] int[] occluded, int flags);
    [DllImport(Lib)] internal static extern int urt_ray_query_device(IntPtr ctx, IntPtr deviceRays, int n, IntPtr deviceOut, int flags);

    // ---- radiance queries (include/urt.h "radiance queries"; records of include/urt_types.h) ---------------------------
    [StructLayout(LayoutKind.Sequential, Pack = 1)]
    internal struct PathRay {                               // urt_PathRay, 48 B
        public float ox, oy, oz, seed;                      // seed: the running _Seed the path's first rand() starts from
        public float dx, dy, dz;
        public int reserved0;
        public float px, py;                                // the "pixel" of rand(): selects the query's random stream
        public int reserved1a, reserved1b;
    }
    [StructLayout(LayoutKind.Sequential, Pack = 1)]
    internal struct PathPixel { public int x, y; }          // urt_PathPixel, 8 B
    internal const int RadianceRays = 0, RadiancePixels = 1;
    [DllImport(Lib)] internal static extern int urt_radiance_query(IntPtr ctx, [In] PathRay[] rays, int n, int samples, int bounces, [Out] float[] outRgba, int flags);
    [DllImport(Lib, EntryPoint = "urt_radiance_query")] internal static extern int urt_radiance_query_pixels(IntPtr ctx, [In] PathPixel[] pixels, int n, int samples, int bounces, [Out] float[] outRgba, int flags);
    [DllImport(Lib)] internal static extern int urt_radiance_query_device(IntPtr ctx, IntPtr deviceIn, int n, int samples, int bounces, IntPtr deviceOutRgba, int flags);

    // ---- feature buffers (include/urt.h "feature buffers"): hit, normal, albedo, id texture handles, 0 = not wanted --------
    internal const int AovPixelCenter = 0, AovFrameRay = 1;
    [DllImport(Lib)] internal static extern int urt_render_aov(IntPtr ctx, ulong hit, ulong normal, ulong albedo, ulong id, int flags);

    // ---- denoising (include/urt.h "denoising"): src, dst, hit, normal, albedo (0 = no demodulation) texture handles --------
    [StructLayout(LayoutKind.Sequential)]
    internal struct DenoiseParams {                         // urt_DenoiseParams, 16 B; a sigma <= 0 leaves its term out
        public int iterations;                              // 1..5
        public float sigmaColor;
        public float sigmaNormal;
        public float sigmaDepth;
    }
    [DllImport(Lib)] internal static extern int urt_denoise(IntPtr ctx, ulong src, ulong dst, ulong hit, ulong normal, ulong albedo, in DenoiseParams p);

    // ---- temporal reprojection (include/urt.h "temporal reprojection"): count textures hold the per-pixel sample count in .x ----
    [StructLayout(LayoutKind.Sequential)]
    internal struct ReprojectParams {                       // urt_ReprojectParams, 80 B
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)]
        public float[] prevWorldToClip;                     // the previous camera's projectionMatrix * worldToCameraMatrix, column-major
        public float maxHistory;                            // 0 = unlimited, else >= 1
        public float normalThreshold;
        public float planeThreshold;
        public int flags;                                   // 0
    }
    [StructLayout(LayoutKind.Sequential)]
    internal struct ReprojectImages {                       // urt_ReprojectImages, 88 B: texture handles, motion 0 = not wanted
        public ulong prevColor, prevCount;
        public ulong prevHit, prevNormal, prevId;
        public ulong hit, normal, id;
        public ulong color, count;
        public ulong motion;
    }
    internal const float ReprojectDefaultMaxHistory = 64.0f, ReprojectDefaultNormalThreshold = 0.9f, ReprojectDefaultPlaneThreshold = 0.02f;
    [DllImport(Lib)] internal static extern int urt_reproject(IntPtr ctx, in ReprojectImages images, in ReprojectParams p);
    [DllImport(Lib)] internal static extern int urt_blit_add_history(IntPtr ctx, ulong src, ulong dst, ulong count, float maxHistory);
    // resampling (include/urt.h "resampling"): devicePixels = urt_PathPixel[], 8-byte aligned; deviceSamples = RGBA32F, 16-byte aligned
    [DllImport(Lib)] internal static extern int urt_select_pixels(IntPtr ctx, ulong count, float below, IntPtr devicePixels, int capacity, out int n);
    [DllImport(Lib)] internal static extern int urt_blend_samples(IntPtr ctx, IntPtr devicePixels, IntPtr deviceSamples, int n, float weight, ulong dst, ulong count, float maxHistory);
    [DllImport(Lib)] internal static extern int urt_resample_below(IntPtr ctx, ulong dst, ulong count, float below, int samples, int bounces, float weight, float maxHistory, out int n);
    // per-object motion (include/urt.h urt_reproject_objects): tables are buffers of urt_buffer_create with stride 48, entry i = object i
    [StructLayout(LayoutKind.Sequential)]
    internal struct ObjectMotion {                          // urt_ObjectMotion, 48 B: current world -> previous world
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 12)]
        public float[] a;                                   // three columns of the linear part, then the translation
    }
    [StructLayout(LayoutKind.Sequential)]
    internal struct ReprojectMotion {                       // urt_ReprojectMotion, 24 B
        public ulong meshMotion, sphereMotion;              // buffer handles; 0 = no object of that kind has moved
        public float movedMaxHistory;                       // 0 = none, else >= 1
        public int flags;                                   // 0
    }
    internal const int ObjectMotionStride = 48;
    [DllImport(Lib)] internal static extern int urt_reproject_objects(IntPtr ctx, in ReprojectImages images, in ReprojectParams p, in ReprojectMotion motion);
    // per-vertex motion (include/urt.h urt_reproject_deformed): the previous positions of meshes that changed shape, kept on the device
    [StructLayout(LayoutKind.Sequential)]
    internal struct ReprojectDeform {                       // urt_ReprojectDeform, 40 B
        public ulong prevVertices, indices, prevMeshObjects, deformed;   // buffer handles: strides 12, 4, 112, 4
        public float normalThreshold;                       // of the per-vertex path; not NaN
        public int flags;                                   // 0
    }
    internal const float ReprojectDefaultDeformNormalThreshold = 0.3f;
    [DllImport(Lib)] internal static extern int urt_reproject_deformed(IntPtr ctx, in ReprojectImages images, in ReprojectParams p, in ReprojectMotion motion, in ReprojectDeform deform);
    [DllImport(Lib)] internal static extern int urt_buffer_copy(IntPtr ctx, ulong src, int srcFirst, ulong dst, int dstFirst, int count);

    // ---- guide-driven upsampling (include/urt.h "guide-driven upsampling"): the low* images have one size, the others another ----
    internal const int UpsampleWideFallback = 1, UpsampleSkyFromAlbedo = 2;
    [StructLayout(LayoutKind.Sequential)]
    internal struct UpsampleParams {                        // urt_UpsampleParams, 16 B
        public float normalThreshold;
        public float planeThreshold;
        public float countScale;                            // finite, > 0
        public int flags;                                   // Upsample*
    }
    [StructLayout(LayoutKind.Sequential)]
    internal struct UpsampleImages {                        // urt_UpsampleImages, 88 B: texture handles; lowCount, albedo, count 0 = not given
        public ulong lowColor, lowCount;
        public ulong lowHit, lowNormal, lowId;
        public ulong hit, normal, id;
        public ulong albedo;
        public ulong color, count;
    }
    internal const float UpsampleDefaultNormalThreshold = 0.9f, UpsampleDefaultPlaneThreshold = 0.02f, UpsampleDefaultCountScale = 1.0f;
    [DllImport(Lib)] internal static extern int urt_upsample(IntPtr ctx, in UpsampleImages images, in UpsampleParams p);

    // ---- auto-exposure and tone mapping (include/urt.h "auto-exposure and tone mapping"): the state lives in device memory ----
    internal const int TonemapLinear = 0, TonemapReinhard = 1, TonemapAces = 2;
    internal const int ExposureStateBytes = 1040;
    [StructLayout(LayoutKind.Sequential)]
    internal struct ExposureState {                         // urt_ExposureState, 1040 B (what a host downloads from its device memory)
        public float exposure;
        public float target;
        public uint counted;
        public uint skipped;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 256)]
        public uint[] hist;
    }
    [StructLayout(LayoutKind.Sequential)]
    internal struct ExposureParams {                        // urt_ExposureParams, 24 B
        public float key;
        public float minExposure;
        public float maxExposure;
        public float rate;
        public int lowPermille;
        public int highPermille;
    }
    [StructLayout(LayoutKind.Sequential)]
    internal struct TonemapParams {                         // urt_TonemapParams, 16 B
        public float exposure;
        public float white;                                 // 0.01 .. 65504
        public int op;                                      // Tonemap*
        public int flags;                                   // 0
    }
    internal const float ExposureDefaultKey = 0.18f, ExposureDefaultMinExposure = 0.015625f, ExposureDefaultMaxExposure = 64.0f, ExposureDefaultRate = 1.0f;
    internal const int ExposureDefaultLowPermille = 100, ExposureDefaultHighPermille = 950;
    internal const float TonemapDefaultExposure = 1.0f, TonemapDefaultWhite = 4.0f;
    internal const int TonemapDefaultOp = TonemapAces, TonemapDefaultFlags = 0;
    [DllImport(Lib)] internal static extern int urt_auto_exposure(IntPtr ctx, ulong src, ulong count, in ExposureParams p, IntPtr dState);
    [DllImport(Lib)] internal static extern int urt_tonemap(IntPtr ctx, ulong src, ulong dst, in TonemapParams p, IntPtr dState);

    // ---- depth of field (include/urt.h "depth of field"): between the metering and the bloom, reads the hit target of urt_render_aov ----
    internal const int DofFlagCoc = 1;
    internal const float DofMaxRadius = 16.0f;
    [StructLayout(LayoutKind.Sequential)]
    internal struct DofParams {                             // urt_DofParams, 16 B
        public float focusDistance;                         // finite, > 0: the hit distance that is sharp
        public float scale;                                 // finite, >= 0: the blur radius in pixels of a point at infinity
        public float maxRadius;                             // 0.5 .. DofMaxRadius
        public int flags;                                   // DofFlag*
    }
    internal const float DofDefaultFocusDistance = 10.0f, DofDefaultScale = 8.0f, DofDefaultMaxRadius = 8.0f;
    internal const int DofDefaultFlags = 0;
    [DllImport(Lib)] internal static extern int urt_depth_of_field(IntPtr ctx, ulong src, ulong hit, ulong dst, in DofParams p);

    // ---- motion blur (include/urt.h "motion blur"): between the depth of field and the bloom, reads the motion image of urt_reproject*
    // and the hit target of urt_render_aov ----
    internal const int MotionBlurFlagVelocity = 1;
    internal const float MotionBlurMaxRadius = 16.0f;
    [StructLayout(LayoutKind.Sequential)]
    internal struct MotionBlurParams {                      // urt_MotionBlurParams, 16 B
        public float shutter;                               // finite, 0 .. 1: the part of the frame interval the shutter is open
        public float maxRadius;                             // 0.5 .. MotionBlurMaxRadius
        public int flags;                                   // MotionBlurFlag*
        public int reserved;                                // 0
    }
    internal const float MotionBlurDefaultShutter = 0.5f, MotionBlurDefaultMaxRadius = 16.0f;
    [DllImport(Lib)] internal static extern int urt_motion_blur(IntPtr ctx, ulong src, ulong motion, ulong hit, ulong dst, in MotionBlurParams p);

    // ---- bloom (include/urt.h "bloom"): between the metering and the tone mapping, reads the same exposure state ----
    internal const int BloomFlagOnly = 1;
    [StructLayout(LayoutKind.Sequential)]
    internal struct BloomParams {                           // urt_BloomParams, 28 B
        public float threshold;                             // 0 .. 65504, in exposed units
        public float softKnee;                              // 0 .. 1
        public float clamp;                                 // > 0 .. 65504, in exposed units
        public float scatter;                               // 0 .. 1
        public float intensity;                             // finite, >= 0
        public int levels;                                  // 1 .. 16
        public int flags;                                   // BloomFlag*
    }
    internal const float BloomDefaultThreshold = 1.0f, BloomDefaultSoftKnee = 0.5f, BloomDefaultClamp = 65504.0f, BloomDefaultScatter = 0.7f, BloomDefaultIntensity = 0.2f;
    internal const int BloomDefaultLevels = 6, BloomDefaultFlags = 0;
    [DllImport(Lib)] internal static extern int urt_bloom(IntPtr ctx, ulong src, ulong dst, in BloomParams p, IntPtr dState);

    // ---- measurement ----------------------------------------------------------------------------------------------------
    [StructLayout(LayoutKind.Sequential)]
    internal struct Counters {
        public ulong rays, tlasNodes, blasNodes, triTests, sphereTests, hitTri, hitSphere, hitGround, hitSky, pixels, dispatches;
        public float traceMs;
        public uint watchdogTrips;
        public ulong launches;
    }
    [DllImport(Lib)] internal static extern int urt_set_option(IntPtr ctx, string name, int value);
    [DllImport(Lib)] internal static extern int urt_get_counters(IntPtr ctx, out Counters c);
    [DllImport(Lib)] internal static extern int urt_reset_counters(IntPtr ctx);

    // ---- device groups: this (single) host thread drives N GPUs                               include/urt.h "device groups"
    [DllImport(Lib)] internal static extern int urt_group_create(int[] devices, int nDevices, out IntPtr group);
    [DllImport(Lib)] internal static extern int urt_group_destroy(IntPtr group);
    [DllImport(Lib)] internal static extern int urt_group_size(IntPtr group);
    [DllImport(Lib)] internal static extern IntPtr urt_group_context(IntPtr group, int rank);
    [DllImport(Lib)] internal static extern IntPtr urt_group_last_error(IntPtr group);
    [DllImport(Lib)] internal static extern int urt_group_buffer_create(IntPtr group, int count, int stride, out ulong buffer);
    [DllImport(Lib)] internal static extern int urt_group_buffer_set_data(IntPtr group, ulong buffer, IntPtr data, int count);
    [DllImport(Lib)] internal static extern int urt_group_buffer_set_data_range(IntPtr group, ulong buffer, int first, IntPtr data, int count);
    [DllImport(Lib)] internal static extern int urt_group_buffer_release(IntPtr group, ulong buffer);
    [DllImport(Lib)] internal static extern int urt_group_texture_create(IntPtr group, int width, int height, out ulong texture);
    [DllImport(Lib)] internal static extern int urt_group_texture_set_pixels(IntPtr group, ulong texture, float[] rgba);
    [DllImport(Lib)] internal static extern int urt_group_texture_get_pixels(IntPtr group, ulong texture, [Out] float[] rgba);
    [DllImport(Lib)] internal static extern int urt_group_texture_release(IntPtr group, ulong texture);
    [DllImport(Lib)] internal static extern int urt_group_shader_set_buffer(IntPtr group, int kernel, string name, ulong buffer);
    [DllImport(Lib)] internal static extern int urt_group_shader_set_texture(IntPtr group, int kernel, string name, ulong texture);
    [DllImport(Lib)] internal static extern int urt_group_shader_set_matrix(IntPtr group, string name, ref UnityEngine.Matrix4x4 m);
    [DllImport(Lib)] internal static extern int urt_group_shader_set_vector(IntPtr group, string name, ref UnityEngine.Vector4 v);
    [DllImport(Lib)] internal static extern int urt_group_shader_set_float(IntPtr group, string name, float v);
    [DllImport(Lib)] internal static extern int urt_group_shader_set_int(IntPtr group, string name, int v);
    [DllImport(Lib)] internal static extern int urt_group_set_option(IntPtr group, string name, int value);
    [DllImport(Lib)] internal static extern int urt_group_shader_dispatch(IntPtr group, int kernel, int gx, int gy, int gz);
    [DllImport(Lib)] internal static extern int urt_group_blit_add(IntPtr group, ulong src, ulong dst, float sample);
    [DllImport(Lib)] internal static extern int urt_group_blit(IntPtr group, ulong src, ulong dst);
    [DllImport(Lib)] internal static extern int urt_group_gather(IntPtr group, ulong srcTexture, ulong dstTexture);
    [DllImport(Lib)] internal static extern int urt_group_flush(IntPtr group);
    [DllImport(Lib)] internal static extern int urt_group_synchronize(IntPtr group);
    [DllImport(Lib)] internal static extern int urt_group_get_counters(IntPtr group, out Counters c);
    [DllImport(Lib)] internal static extern int urt_group_reset_counters(IntPtr group);

    // ---- host-side helpers (no GPU): normals, object-level heaps, .hdr loader, frame writers, debug log -------------------
    [DllImport(Lib)] internal static extern int urt_host_compute_normals(IntPtr vertices, int nVertices, IntPtr indices, int nIndices, IntPtr outNormals);
    [DllImport(Lib)] internal static extern int urt_host_mesh_leaf_bounds(IntPtr meshObjects, int nMeshes, IntPtr vertices, int nVertices, IntPtr indices, int nIndices, int literal, IntPtr outLeaves);
    [DllImport(Lib)] internal static extern int urt_host_sphere_leaf_bounds(IntPtr spheres, int nSpheres, int literal, IntPtr outLeaves);
    [DllImport(Lib)] internal static extern int urt_host_object_bvh_length(int nObjects);   // < 0 (more than 2^30 objects): treat as URT_ERR_INVALID_ARGUMENT, as both builders do
    [DllImport(Lib)] internal static extern int urt_host_build_object_bvh(IntPtr leaves, int nObjects, IntPtr outNodes, int capacity);
    [DllImport(Lib)] internal static extern int urt_host_load_hdr(string path, out int width, out int height, [Out] float[] rgba, UIntPtr capacityFloats);
    [DllImport(Lib)] internal static extern int urt_host_write_pfm(string path, float[] rgba, int width, int height);
    [DllImport(Lib)] internal static extern int urt_host_write_png(string path, float[] rgba, int width, int height);
    [DllImport(Lib)] internal static extern int urt_host_encode_srgb8(float[] rgba, UIntPtr nPixels, byte[] outRgba8);
    [DllImport(Lib)] internal static extern int urt_host_srgb8_first_floats(float[] out256);
    [DllImport(Lib)] internal static extern int urt_host_log(string path, int debugLevel, int level, string text);
    [DllImport(Lib)] internal static extern int urt_host_log_scene_counts(string path, int debugLevel, int nSpheres, int nMeshObjects, int nVertices, int nIndices, int nNormals);
    [DllImport(Lib)] internal static extern int urt_host_log_tree_report(string path, int debugLevel, int nMeshObjects, int meshDepth, int meshRealLength, int nSpheres, int sphereDepth, int sphereRealLength);
    [DllImport(Lib)] internal static extern int urt_host_dump_bvh(string path, IntPtr nodes, int nNodes, int depth, float[] rayStart3, float[] rayEnd3, out int lines);
    [DllImport(Lib)] internal static extern int urt_host_dump_normals(string path, IntPtr meshObjects, int nMeshes, float[] vertices, int nVertices, int[] indices, int nIndices, float[] normals, int nNormals, out int lines);
    [DllImport(Lib)] internal static extern int urt_debug_refit_stats(IntPtr ctx, out ulong refittedMeshes, out ulong incrementalPreparations);
    [DllImport(Lib)] internal static extern int urt_debug_deform_stats(IntPtr ctx, [Out] ulong[] out6);   // deformed, renormed, bytes copied, forced rebuilds, cost-ratio float bits, 0
    [DllImport(Lib)] internal static extern int urt_debug_scene_cost(IntPtr ctx, [Out] float[] out2PerMesh, int nMeshes);
    [DllImport(Lib)] internal static extern int urt_debug_scene_vertex_spans(IntPtr ctx, [Out] int[] outLo, [Out] int[] outHi, int nMeshes);   // INT32_MAX / -1: none
    [DllImport(Lib)] internal static extern int urt_debug_prepare_stats(IntPtr ctx, [Out] ulong[] out4);   // full preparations, device-fed ones, span chunk, span ms float bits
    [DllImport(Lib)] internal static extern int urt_debug_live_resources([Out] ulong[] out4);   // process-wide: device bytes, pinned bytes, events, streams
    [DllImport(Lib)] internal static extern int urt_host_mesh_motion(IntPtr prevMeshObjects, IntPtr curMeshObjects, int n, IntPtr outMotion);   // 48 B per entry
    [DllImport(Lib)] internal static extern int urt_host_sphere_motion(IntPtr prevSpheres, IntPtr curSpheres, int n, IntPtr outMotion);
    [DllImport(Lib)] internal static extern int urt_host_build_object_bvh_pairing(IntPtr leaves, int nObjects, IntPtr outNodes, int capacity);   // RM:459-722's pairing builder, restated
    [DllImport(Lib)] internal static extern int urt_host_resize_rgba(float[] src, int width, int height, [Out] float[] dst, int newWidth, int newHeight);
    [DllImport(Lib)] internal static extern IntPtr urt_host_last_error();          // const char* (thread-local, like the two below)
    [DllImport(Lib)] internal static extern IntPtr urt_host_io_last_error();
    [DllImport(Lib)] internal static extern IntPtr urt_host_debug_last_error();
    // ---- introspection (what tests/ use; not needed by RM) --------------------------------------------------------------
    [DllImport(Lib)] internal static extern int urt_debug_build_blas(IntPtr meshObjects, int nMeshes, float[] vertices, int nVertices, int[] indices, int nIndices, out int nNodes, out int nTris, out int maxDepth);
    [DllImport(Lib)] internal static extern int urt_debug_get_blas([Out] float[] nodes, [Out] int[] triIndex, [Out] int[] meshRoot, [Out] int[] meshFirstTri);
    [DllImport(Lib)] internal static extern int urt_debug_scene_info(IntPtr ctx, out int nNodes, out int nTris, out int maxDepth, out float prepareMs);
    [DllImport(Lib)] internal static extern int urt_debug_launch_info(IntPtr ctx, [Out] byte[] launchInfo208);   // urt_launch_info: char kernel[96] + 28 ints
    [DllImport(Lib)] internal static extern int urt_debug_read_scene_blas(IntPtr ctx, [Out] float[] nodes, [Out] int[] triIndex, [Out] int[] meshRoot);
    [DllImport(Lib)] internal static extern int urt_debug_read_scene_qnodes(IntPtr ctx, [Out] float[] qnodes, out int nNodes, out int inUse);
    [DllImport(Lib)] internal static extern int urt_debug_read_tile_entry(IntPtr ctx, [Out] int[] words, ulong capacityWords, out int tilesX, out int tilesY, out int k, out ulong builds);
    [DllImport(Lib)] internal static extern int urt_debug_read_scene_cones(IntPtr ctx, [Out] uint[] words, [Out] float[] triEdges, out int inUse);
    [DllImport(Lib)] internal static extern int urt_debug_blas_cache_stats(IntPtr ctx, out ulong reused, out ulong built);
    [DllImport(Lib)] internal static extern int urt_debug_serve_stats(IntPtr ctx, [Out] ulong[] out6);
    [DllImport(Lib)] internal static extern int urt_debug_build_walk_table(IntPtr heap, int nNodes, int nMeshes, int[] meshRoot, int[] smallFirst, float[] table, int capacityWords, out int words);

    // Unity's own API returns void and logs on error: the shim keeps that behaviour.
    internal static void Check(IntPtr ctx, int rc) {
        if (rc != 0) UnityEngine.Debug.LogError("urt: " + Marshal.PtrToStringAnsi(urt_last_error(ctx)));
    }
    internal static void CheckGroup(IntPtr group, int rc) {
        if (rc != 0) UnityEngine.Debug.LogError("urt group: " + Marshal.PtrToStringAnsi(urt_group_last_error(group)));
    }
}
