// upsample.h — host-callable launcher of the guide-driven upsampling (upsample.hip): urt_upsample
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace urtd {

// The images of one urt_upsample call: RGBA32F, row 0 = bottom (the urt_render_aov layouts; a count texel holds the per-pixel sample
// count in .x).  The low_* images are low_width x low_height, the others width x height.
struct UpsampleImages {
  const float4* low_color;      // the image traced on the low grid
  const float4* low_count;      // or null: every texel counts 1.0f
  const float4* low_hit;        // urt_render_aov(URT_AOV_PIXEL_CENTER) on the low grid: position.xyz, distance
  const float4* low_normal;     // normal.xyz, kind
  const float4* low_id;         // object (int bits), ...
  const float4* hit;            // the same on the full grid, same camera
  const float4* normal;
  const float4* id;
  const float4* albedo;         // or null: read for sky pixels only, with URT_UPSAMPLE_SKY_FROM_ALBEDO
  float4* color;                // out: the reconstructed image
  float4* count;                // out or null: (count, 0, 0, 0)
  int low_width, low_height, width, height;
};

// include/urt.h urt_UpsampleParams, already checked.
struct UpsampleSettings {
  float normal_threshold, plane_threshold, count_scale;
  int wide_fallback;            // URT_UPSAMPLE_WIDE_FALLBACK: stage 2 for pixels stage 1 leaves without a result
  int sky_from_albedo;          // URT_UPSAMPLE_SKY_FROM_ALBEDO
};

// Enqueues k_upsample on `st`.  hipErrorInvalidValue when the grid is too tall.
hipError_t launch_upsample(const UpsampleImages& I, const UpsampleSettings& P, hipStream_t st);

}  // namespace urtd
