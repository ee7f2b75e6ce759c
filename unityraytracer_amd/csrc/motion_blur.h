// motion_blur.h — host-callable launcher of the motion-blur kernels (motion_blur.hip): urt_motion_blur
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace urtd {

constexpr int kMotionBlurMaxReach = 16;           // include/urt.h URT_MOTION_BLUR_MAX_RADIUS: no tap lies further than this along an axis
constexpr int kMotionBlurMaxExtent = 1 << 30;     // width and height the kernels' int coordinates (x + 16) are good for

// include/urt.h urt_MotionBlurParams, already checked
struct MotionBlurSettings {
  float shutter, max_radius;
  int flags;                                      // URT_MOTION_BLUR_FLAG_*
};

// The scratch of one call, in floats: {v.x, v.y, m, 0} of each 16 x 16 tile (first: the records are read as float4), then {l, z} per pixel.
inline size_t motion_blur_tiles(int width, int height) { return (size_t)((width + 15) / 16) * (size_t)((height + 15) / 16); }
inline size_t motion_blur_scratch_floats(int width, int height) {
  return 4 * motion_blur_tiles(width, height) + 2 * (size_t)width * (size_t)height;
}

// Enqueues on `st` the kernels of one urt_motion_blur call: k_mb_velocity (class, velocity and tile table into the scratch), then
// k_mb_gather into dst (with URT_MOTION_BLUR_FLAG_VELOCITY it writes the neighbourhood velocity instead of the image).  scratch:
// motion_blur_scratch_floats(..) floats of device memory, 16-byte aligned; nothing in it is read before this call wrote it.  dst is none
// of src, motion and hit.  width, height in 1..kMotionBlurMaxExtent, (height + 15) / 16 <= 65535 (hipErrorInvalidValue otherwise,
// nothing enqueued).
hipError_t launch_motion_blur(const float4* src, const float4* motion, const float4* hit, float4* dst, int width, int height,
                              const MotionBlurSettings& P, float* scratch, hipStream_t st);

}  // namespace urtd
