// skin.h — linear blend skinning into vertex buffers and the finite bounds of a stride-12 buffer (csrc/skin.hip).  Private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace urtd {

// bones up to this count are staged in LDS (48 B each: 12 KiB of a workgroup's LDS); a larger table is gathered from global memory
constexpr int kSkinLdsBones = 256;
constexpr int kSkinBlock = 256;              // vertices per workgroup, one per lane
constexpr int kBoundsMaxBlocks = 1024;       // partials of the first bounds pass
constexpr int kBoundsWords = 8;              // min.xyz, max.xyz, count (as bits), 0

// include/urt.h urt_skin_vertices: elements first .. first + count - 1 (count > 0).  rest_n / dst_n NULL: positions only.
hipError_t skin_vertices(const float* rest_v, const float* rest_n, const int32_t* bone_idx, const float* bone_wgt, const float* bones,
                         int n_bones, int first, int count, float* dst_v, float* dst_n, hipStream_t st);
// include/urt.h urt_buffer_bounds: partial must hold kBoundsMaxBlocks * kBoundsWords floats, out kBoundsWords (count > 0)
hipError_t buffer_bounds(const float* v, int first, int count, float* partial, float* out, hipStream_t st);

}  // namespace urtd
