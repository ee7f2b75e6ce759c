// normals.hip — vertex normals recomputed on the device, as RayTraceMaster.ComputeNormals (RM:340-368) defines them:
//   k_face_normals     the un-normalised normal of every triangle a plan needs, 16 bytes per face
//   k_vertex_normals   per served vertex the sum of its contributing faces IN THE PLAN'S ORDER, normalised
// Plain stores, then an inverted index read in a fixed order: no atomics, and one vertex's sum is never split across lanes — float
// addition does not commute in rounding, and the ascending slot order is the specification.  The arithmetic is NORMATIVE
// (include/urt.h urt_compute_normals; tests/normals_ref.py restates it in numpy): float32, one rounding per operation, evaluated as
// written, no fma.  Built with -ffp-contract=off like every normative kernel.
#include "normals.h"

#include "../../include/urt_math.h"

namespace {

using urtd::kNormalsBlock;

// One needed triangle per lane: face = cross(b - a, c - a), gathered from the vertices buffer's mirror through the plan's own triangles.
__global__ __launch_bounds__(kNormalsBlock) void k_face_normals(const float* __restrict__ v, const int32_t* __restrict__ tris, int n_tris,
                                                                float4* __restrict__ face) {
  const long long t = (long long)blockIdx.x * kNormalsBlock + (long long)threadIdx.x;
  if (t >= (long long)n_tris) return;
  const size_t ia = 3 * (size_t)tris[3 * (size_t)t], ib = 3 * (size_t)tris[3 * (size_t)t + 1], ic = 3 * (size_t)tris[3 * (size_t)t + 2];
  const float ax = v[ia], ay = v[ia + 1], az = v[ia + 2];
  const float e1x = v[ib] - ax, e1y = v[ib + 1] - ay, e1z = v[ib + 2] - az;
  const float e2x = v[ic] - ax, e2y = v[ic + 1] - ay, e2z = v[ic + 2] - az;
  face[(size_t)t] = make_float4(e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x, 0.0f);
}

// One served vertex per lane, kNormalsBlock per workgroup.  A lane walks its list sequentially (a high-valence vertex makes its lane's
// loop longer: accepted); one face is one 16-byte load.  The results leave like k_skin's: turned in LDS at a stride of 3 dwords
// (conflict-free) and stored dword by dword, so every wave store covers whole cache lines of the stride-12 destination whatever `first`
// is; only the last block is ragged.
__global__ __launch_bounds__(kNormalsBlock) void k_vertex_normals(const int2* __restrict__ ranges, const int32_t* __restrict__ entries,
                                                                  const float4* __restrict__ face, int first, int count,
                                                                  float* __restrict__ dst) {
  __shared__ float s_n[3 * kNormalsBlock];
  const int tid = (int)threadIdx.x;
  const long long block_rel = (long long)blockIdx.x * kNormalsBlock;               // the block's first served vertex, relative to `first`
  const long long left = (long long)count - block_rel;
  const int in_block = left < (long long)kNormalsBlock ? (int)left : kNormalsBlock;  // >= 1: the grid is ceil(count / kNormalsBlock)
  if (tid < in_block) {
    const int2 r = ranges[(size_t)block_rel + (size_t)tid];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int k = 0; k < r.y; k++) {
      const float4 f = face[(size_t)entries[(size_t)r.x + (size_t)k]];
      sx = sx + f.x; sy = sy + f.y; sz = sz + f.z;
    }
    const float mag = urt::f_sqrt((sx * sx + sy * sy) + sz * sz);
    const bool keep = mag > 1e-5f;                                                 // (a NaN magnitude fails the comparison)
    s_n[3 * tid] = keep ? sx / mag : 0.0f;
    s_n[3 * tid + 1] = keep ? sy / mag : 0.0f;
    s_n[3 * tid + 2] = keep ? sz / mag : 0.0f;
  }
  __syncthreads();
  const size_t base = ((size_t)first + (size_t)block_rel) * 3;
  for (int k = tid; k < 3 * in_block; k += kNormalsBlock) dst[base + (size_t)k] = s_n[k];
}

}  // namespace

namespace urtd {

hipError_t compute_normals(const float* vertices, const int32_t* tris, int n_tris, const int32_t* ranges, const int32_t* entries,
                           int first, int count, float4* face, float* dst, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  const dim3 block(kNormalsBlock);
  if (n_tris > 0) {
    const dim3 grid((unsigned int)(((long long)n_tris + kNormalsBlock - 1) / kNormalsBlock));
    hipLaunchKernelGGL(k_face_normals, grid, block, 0, st, vertices, tris, n_tris, face);
  }
  const dim3 grid((unsigned int)(((long long)count + kNormalsBlock - 1) / kNormalsBlock));
  hipLaunchKernelGGL(k_vertex_normals, grid, block, 0, st, (const int2*)ranges, entries, (const float4*)face, first, count, dst);
  return hipGetLastError();
}

}  // namespace urtd
