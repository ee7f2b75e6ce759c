// dof.h — host-callable launcher of the depth-of-field kernels (dof.hip): urt_depth_of_field
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace urtd {

constexpr int kDofMaxReach = 16;           // include/urt.h URT_DOF_MAX_RADIUS: no tap further than this along an axis can count
constexpr int kDofMaxExtent = 1 << 30;     // width and height the kernels' int coordinates (x + 32) are good for

// include/urt.h urt_DofParams, already checked
struct DofSettings {
  float focus_distance, scale, max_radius;
  int flags;                               // URT_DOF_FLAG_*
};

// The scratch of one call, in floats: {a, z} per pixel, then the largest a of each 16 x 16 tile.
inline size_t dof_tiles(int width, int height) { return (size_t)((width + 15) / 16) * (size_t)((height + 15) / 16); }
inline size_t dof_scratch_floats(int width, int height) { return 2 * (size_t)width * (size_t)height + dof_tiles(width, height); }

// Enqueues on `st` the kernels of one urt_depth_of_field call: k_dof_coc (class, blur radius and tile table into the scratch), then
// k_dof_gather into dst; with URT_DOF_FLAG_COC k_dof_coc writes dst itself and nothing follows.  scratch: dof_scratch_floats(..)
// floats of device memory, 8-byte aligned; nothing in it is read before this call wrote it.  dst is neither src nor hit.  width, height in 1..kDofMaxExtent,
// (height + 15) / 16 <= 65535 (hipErrorInvalidValue otherwise, nothing enqueued).
hipError_t launch_depth_of_field(const float4* src, const float4* hit, float4* dst, int width, int height, const DofSettings& P,
                                 float* scratch, hipStream_t st);

}  // namespace urtd
