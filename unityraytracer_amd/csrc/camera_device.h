// camera_device.h — the camera ray of a pixel, CreateCameraRay RS:142-153 with the uv of RS:448-449: the ONE place it is written, for the
// frame kernels (frame_device.h camera_ray / camera_ray_frame), the feature buffers (aov.hip) and the radiance queries (radiance.hip).
// The order of the floating-point operations is normative.  Uniforms come by reference and matrices behind a pointer of any address
// space (a plain const float*, the kernel-argument segment, the frame table): each caller's loads stay where its expression uses them.
// Internal to the library; included by .hip translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/urt_math.h"

namespace {

// one axis of the uv in [-1, 1]: the sample position s, in pixels, on an image `extent` pixels wide or high
__device__ __forceinline__ float axis_uv(float s, const int& extent) { return s / (float)extent * 2.0f - 1.0f; }

// RS:448-449: the next two rand() draws of pixel (px, py) and _PixelOffset place the sample; the seed carries over (RS:444)
__device__ __forceinline__ void jitter_uv(float& seed, float px, float py, const float& off_x, const float& off_y, const int& width,
                                          const int& height, float& u, float& v) {
  float r0 = urt::rand_next(seed, px, py);
  float r1 = urt::rand_next(seed, px, py);
  u = axis_uv(px + r0 + off_x, width);
  v = axis_uv(py + r1 + off_y, height);
}

// urt::mul_m4 on a matrix behind any pointer type M
template <typename M>
__device__ __forceinline__ urt::v3 mul_m4_k(M m, float x, float y, float z, float w) {
  urt::v3 r;
  r.x = urt::f_fma(m[12], w, urt::f_fma(m[8], z, urt::f_fma(m[4], y, m[0] * x)));
  r.y = urt::f_fma(m[13], w, urt::f_fma(m[9], z, urt::f_fma(m[5], y, m[1] * x)));
  r.z = urt::f_fma(m[14], w, urt::f_fma(m[10], z, urt::f_fma(m[6], y, m[2] * x)));
  return r;
}
// CreateCameraRay RS:142-153
template <typename M>
__device__ __forceinline__ void camera_ray_uv(M c2w, M invp, float u, float v, urt::v3& o, urt::v3& d) {
  o = mul_m4_k(c2w, 0.0f, 0.0f, 0.0f, 1.0f);
  urt::v3 dir = mul_m4_k(invp, u, v, 0.0f, 1.0f);
  dir = mul_m4_k(c2w, dir.x, dir.y, dir.z, 0.0f);
  d = urt::normalize(dir);
}

}  // namespace
