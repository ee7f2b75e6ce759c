// morph.h — blend shapes (morph targets) applied to a range of vertices and normals (csrc/morph.hip).  Private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace urtd {

constexpr int kMorphBlock = 256;             // served vertices per workgroup, one per lane

// include/urt.h urt_morph_vertices: the plan's served vertices first .. first + count - 1 (count > 0).  ranges: {start, length} per
// served vertex into targets / deltas; targets: one int32 per entry, each inside the weight table; deltas: 6 floats per entry (dp, dn).
// rest_n / dst_n NULL: positions only (normalize is ignored then).
hipError_t morph_vertices(const float* rest_v, const float* rest_n, const int32_t* ranges, const int32_t* targets, const float* deltas,
                          const float* weights, int first, int count, float* dst_v, float* dst_n, bool normalize, hipStream_t st);

}  // namespace urtd
