// radiance.h — host-callable launcher of the batched radiance queries (radiance.hip): urt_radiance_query / urt_radiance_query_device
#pragma once
#include <hip/hip_runtime.h>
#include "urt_device.h"

namespace urtd {

// One batch.  in: n urt_PathRay (3 float4 each, 16-byte aligned) or, with `pixels`, n urt_PathPixel (8 bytes each, 8-byte aligned);
// out: n float4.  width, height: pixels mode, the size of the texture bound as Result (Result.GetDimensions); rays mode reads neither.
// work_counter: null = one query per thread of the grid (k_radiance); else a device word of this launch's own (it is zeroed on `st` in
// front of the kernel) from which a resident grid — as many workgroups as fit n_cus compute units at once — draws the query indices
// (k_radiance_persist).
struct RadianceBatch {
  const void* in; float4* out;
  int n, samples, bounces;
  bool pixels; int width, height;
  unsigned int* work_counter; int n_cus;
};

// E: LDS entries per lane of the prepared scene (as launch_query).  S.sky must be set.  C: pixels mode, the uniforms bound at call time
// (RS:5-7, 16); rays mode reads none of it.
hipError_t launch_radiance(const DevScene& S, LaneStackSize E, const FrameUniforms& C, const RadianceBatch& B, hipStream_t st);

}  // namespace urtd
