// normals.h — RayTraceMaster.ComputeNormals over a plan, on the device (csrc/normals.hip; the plan: csrc/normals_plan.h).  Private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace urtd {

constexpr int kNormalsBlock = 256;           // triangles / served vertices per workgroup, one per lane

// include/urt.h urt_compute_normals: the un-normalised face normals of the plan's n_tris triangles (tris: 3 vertex indices each, all
// inside `vertices`) into face[0 .. n_tris - 1], then the served vertices first .. first + count - 1 (count > 0) into dst: ranges holds
// {start, length} into entries per served vertex, entries positions in `face`.
hipError_t compute_normals(const float* vertices, const int32_t* tris, int n_tris, const int32_t* ranges, const int32_t* entries,
                           int first, int count, float4* face, float* dst, hipStream_t st);

}  // namespace urtd
