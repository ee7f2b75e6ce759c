// query.h — host-callable launcher of the batched ray queries (query.hip): urt_ray_query / urt_ray_query_device
#pragma once
#include <hip/hip_runtime.h>
#include "urt_device.h"

namespace urtd {

// rays: 2 float4 per ray (urt_Ray: origin.xyz, t_max | direction.xyz, reserved), 16-byte aligned.
// any_hit = false: out = 3 float4 per ray (urt_RayHit); true: out = one int32 per ray (1 = occluded).
// E: LDS entries per lane of the prepared scene (context_impl.h lane_stack_size).
hipError_t launch_query(const DevScene& S, LaneStackSize E, const float4* rays, int n, void* out, bool any_hit, hipStream_t st);

}  // namespace urtd
