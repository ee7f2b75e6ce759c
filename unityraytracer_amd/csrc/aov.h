// aov.h — host-callable launcher of the per-pixel first-hit feature buffers (aov.hip): urt_render_aov
#pragma once
#include <hip/hip_runtime.h>
#include "urt_device.h"

namespace urtd {

// The camera of one urt_render_aov call: the uniforms bound at call time (RS:5-7, 16).  frame_ray = 0: the pixel-centre ray; 1: the
// first camera ray (sample 0) of a frame dispatched now (RS:448-449 with _Seed and _PixelOffset).
struct AovCamera {
  float c2w[16];            // _CameraToWorld
  float invp[16];           // _CameraInverseProjection
  float pixel_off_x, pixel_off_y;   // _PixelOffset
  float seed;               // _Seed
  int frame_ray;
};

// The targets: RGBA32F images of width x height (row 0 = bottom), or null when not wanted.
struct AovTargets {
  float4* hit;              // position.xyz, distance
  float4* normal;           // normal.xyz, kind as a float value
  float4* albedo;           // clamped albedo.xyz, smoothness; a miss: sky radiance, 0
  float4* id;               // object, primitive (int bits), u | v
  int width, height;
};

// albedo: one float4 per material in the order of DevScene::materials (spheres, MeshObjects, ground): min(1 - specular, albedo), smoothness.
// tlas_stack / blas_stack: LDS entries per lane of the prepared scene (as launch_query).  S.sky must be set (the frame kernels' sky).
hipError_t launch_aov(const DevScene& S, const float4* albedo, int tlas_stack, int blas_stack, const AovCamera& C, const AovTargets& T,
                      hipStream_t st);

}  // namespace urtd
