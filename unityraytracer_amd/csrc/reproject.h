// reproject.h — host-callable launchers of the temporal reprojection (reproject.hip): urt_reproject, urt_reproject_objects,
// urt_reproject_deformed and urt_blit_add_history
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace urtd {

// The images of one urt_reproject call: RGBA32F, width x height, row 0 = bottom (the urt_render_aov layouts; a count texel holds the
// per-pixel sample count in .x).
struct ReprojectImages {
  const float4* prev_color;     // the history under the previous camera
  const float4* prev_count;
  const float4* prev_hit;       // urt_render_aov(URT_AOV_PIXEL_CENTER) under the previous camera: position.xyz, distance
  const float4* prev_normal;    // normal.xyz, kind
  const float4* prev_id;        // object (int bits), ...
  const float4* hit;            // the same under the current camera
  const float4* normal;
  const float4* id;
  float4* color;                // out: the reprojected history
  float4* count;                // out: (count, 0, 0, 0)
  float4* motion;               // out or null: (qx - x, qy - y, S, 0)
  int width, height;
};

// The matrices and thresholds (include/urt.h urt_ReprojectParams plus the current camera uniforms), already checked.
struct ReprojectSettings {
  float m[16];                  // prev_world_to_clip, column-major
  float c2w[16];                // _CameraToWorld
  float invp[16];               // _CameraInverseProjection
  float max_history, normal_threshold, plane_threshold;
};

// The per-object motion tables of urt_reproject_objects: entries of 48 bytes (include/urt.h urt_ObjectMotion) at 16-byte aligned
// device addresses, read as three float4; null = that kind of object has not moved.
struct ReprojectMotion {
  const float4* mesh;           // entry i = MeshObject i
  const float4* sphere;
  int n_mesh, n_sphere;         // entries of each table
  float moved_max_history;      // 0 = none
};

// The buffers of urt_reproject_deformed (include/urt.h urt_ReprojectDeform), as device addresses with their element counts: every index
// the kernel forms is checked against them.  flags null = no deform given (the call is then urt_reproject_objects' pixel for pixel).
struct ReprojectDeform {
  const float* vertices;        // prev_vertices: n_vertices elements of 12 bytes, object space
  const int* indices;           // the buffer bound as _Indices
  const float4* objects;        // prev_mesh_objects: n_objects elements of 112 bytes (7 float4), localToWorldMatrix in the first four
  const int* flags;             // deformed: n_objects int32, nonzero = per-vertex path
  int n_vertices, n_indices, n_objects;
  float normal_threshold;       // of the per-vertex path
};

// Enqueues k_reproject on `st`.  hipErrorInvalidValue when the grid is too tall.
hipError_t launch_reproject(const ReprojectImages& I, const ReprojectSettings& P, hipStream_t st);

// The same with the tables: enqueues k_reproject_objects.
hipError_t launch_reproject_objects(const ReprojectImages& I, const ReprojectSettings& P, const ReprojectMotion& T, hipStream_t st);

// The same with the previous vertex positions of deformed meshes: enqueues k_reproject<true, ParamsDeform>.
hipError_t launch_reproject_deformed(const ReprojectImages& I, const ReprojectSettings& P, const ReprojectMotion& T, const ReprojectDeform& D,
                                     hipStream_t st);

// One AdditionShader blend with the per-pixel sample count of `count` (urt_blit_add_history), in place on dst and count.
hipError_t launch_blit_add_history(const float4* src, float4* dst, float4* count, size_t n_pixels, float max_history, hipStream_t st);

// n consecutive such blends of the frames src + f * frame_stride (f = 0 .. n-1) in one pass, with the same per-pixel operations in the
// same order as n launch_blit_add_history calls; `present` (or null) also receives the final dst value (the present of RM:819).
hipError_t launch_blit_add_history_multi(const float4* src, size_t frame_stride, int n, float4* dst, float4* count, float4* present,
                                         size_t n_pixels, float max_history, hipStream_t st);

}  // namespace urtd
