// bloom.h — host-callable launcher of the bloom kernels (bloom.hip): urt_bloom
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tonemap.h"

namespace urtd {

constexpr int kBloomMaxLevels = 16;        // include/urt.h urt_BloomParams.levels
constexpr int kBloomMaxExtent = 1 << 30;   // width and height the kernels' int coordinates (2x + 2) are good for

// include/urt.h urt_BloomParams, already checked
struct BloomSettings {
  float threshold, soft_knee, clamp, scatter, intensity;
  int levels, flags;                       // URT_BLOOM_FLAG_*
};

// The levels of one call (include/urt.h "level sizes"): level 0 is the image, which is never stored; level l = 1..L has w[l] x h[l]
// texels and starts `offset[l]` float4 into the pyramid; `texels` is the sum over 1..L.
struct BloomLevels {
  int L;
  int w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
  size_t offset[kBloomMaxLevels + 1];
  size_t texels;
};
BloomLevels bloom_levels(int width, int height, int levels);

// Enqueues on `st` the 2L kernels of one urt_bloom call: the prefiltering downsample of src into level 1, the downsamples to level L, the
// upsamples back to level 1 (in place in the pyramid) and the composite into dst.  pyramid: bloom_levels(..).texels float4 of device
// scratch; nothing in it is read before this call wrote it.  dst may be src.  width, height in 1..kBloomMaxExtent,
// (height + 15) / 16 <= 65535 (hipErrorInvalidValue otherwise, nothing enqueued).
hipError_t launch_bloom(const float4* src, float4* dst, int width, int height, const BloomSettings& P, const ExposureState* state,
                        float4* pyramid, hipStream_t st);

}  // namespace urtd
