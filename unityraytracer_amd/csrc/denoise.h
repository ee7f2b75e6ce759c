// denoise.h — host-callable launcher of the edge-aware a-trous denoiser (denoise.hip): urt_denoise
#pragma once
#include <hip/hip_runtime.h>

namespace urtd {

// The images of one urt_denoise call: RGBA32F, width x height, row 0 = bottom (the urt_render_aov layouts).
struct DenoiseImages {
  const float4* src;        // colour.rgb, alpha
  float4* dst;              // may equal src
  const float4* hit;        // position.xyz, distance (the depth z)
  const float4* normal;     // normal.xyz, kind
  const float4* albedo;     // albedo.rgb or null: no demodulation
  float4* scratch;          // 3 * width * height float4: guide, two colour images
  int width, height;
};

// The filter settings (include/urt.h urt_DenoiseParams), already checked: iterations 1..5, no NaN.
struct DenoiseSettings {
  int iterations;
  float sigma_color, sigma_normal, sigma_depth;
};

// Enqueues the pack pass and `iterations` filter passes on `st`.  hipErrorInvalidValue when the grid is too tall.
hipError_t launch_denoise(const DenoiseImages& I, const DenoiseSettings& P, hipStream_t st);

}  // namespace urtd
