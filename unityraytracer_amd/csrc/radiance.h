// radiance.h — host-callable launcher of the batched radiance queries (radiance.hip): urt_radiance_query / urt_radiance_query_device
#pragma once
#include <hip/hip_runtime.h>
#include "urt_device.h"

namespace urtd {

// Pixels mode: the uniforms bound at call time (RS:5-7, 16) and the size of the texture bound as Result.  Rays mode reads none of it.
struct RadianceCamera {
  float c2w[16];            // _CameraToWorld
  float invp[16];           // _CameraInverseProjection
  float pixel_off_x, pixel_off_y;   // _PixelOffset
  float seed;               // _Seed
  int width, height;        // Result.GetDimensions
};

// One batch.  in: n urt_PathRay (3 float4 each, 16-byte aligned) or, with `pixels`, n urt_PathPixel (8 bytes each, 8-byte aligned);
// out: n float4.  tlas_stack / blas_stack: LDS entries per lane of the prepared scene (as launch_query).  S.sky must be set.
// work_counter: null = one query per thread of the grid (k_radiance); else a device word of this launch's own (it is zeroed on `st` in
// front of the kernel) from which a resident grid — as many workgroups as fit n_cus compute units at once — draws the query indices
// (k_radiance_persist).
struct RadianceBatch {
  const void* in; float4* out;
  int n, samples, bounces;
  bool pixels;
  unsigned int* work_counter; int n_cus;
};

hipError_t launch_radiance(const DevScene& S, int tlas_stack, int blas_stack, const RadianceCamera& C, const RadianceBatch& B, hipStream_t st);

}  // namespace urtd
