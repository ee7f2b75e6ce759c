// aov.h — host-callable launcher of the per-pixel first-hit feature buffers (aov.hip): urt_render_aov
#pragma once
#include <hip/hip_runtime.h>
#include "urt_device.h"

namespace urtd {

// The targets: RGBA32F images of width x height (row 0 = bottom), or null when not wanted.
struct AovTargets {
  float4* hit;              // position.xyz, distance
  float4* normal;           // normal.xyz, kind as a float value
  float4* albedo;           // clamped albedo.xyz, smoothness; a miss: sky radiance, 0
  float4* id;               // object, primitive (int bits), u | v
  int width, height;
};

// albedo: one float4 per material in the order of DevScene::materials (spheres, MeshObjects, ground): min(1 - specular, albedo), smoothness.
// E: LDS entries per lane of the prepared scene (as launch_query).  S.sky must be set (the frame kernels' sky).  C: the uniforms bound at
// call time (RS:5-7, 16).  frame_ray = false: the pixel-centre ray; true: the first camera ray (sample 0) of a frame dispatched now
// (RS:448-449 with _Seed and _PixelOffset).
hipError_t launch_aov(const DevScene& S, const float4* albedo, LaneStackSize E, const FrameUniforms& C, bool frame_ray, const AovTargets& T,
                      hipStream_t st);

}  // namespace urtd
