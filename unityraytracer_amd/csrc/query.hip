// query.hip — batched ray queries against the prepared device scene (urt_ray_query / urt_ray_query_device, include/urt.h).
//
// One ray per lane, wave64, 256 threads per workgroup; per-lane LDS stacks (trace_device.h lane_stacks) sized from the prepared scene.
// The walk is trace_device.h trace_ray, the function the frame kernels' Trace is, with the two things a query adds to it:
//  * best.t starts at the ray's t_max, so a hit counts only when t < t_max (exclusive); the object-level cull still compares with the
//    ground-plane distance alone, so its argument does not depend on t_max;
//  * the any-hit form returns at the first hit with 0 < t < t_max (ground plane, a leaf's triangles, a sphere).
// Loads are two float4 per ray, stores three float4 per ray (urt_RayHit) or one int32 (occlusion).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "trace_device.h"
#include "query_device.h"   // hit_record (shared with aov.hip)
#include "query.h"
#include "launch_host.h"

namespace {

// out: 3 float4 per ray = urt_RayHit { distance, position.xyz | normal.xyz, kind | object, primitive, u, v } (ints as bits)
template <bool ANY>
__global__ __launch_bounds__(256) void k_query(DevScene S, int tlas_stack, int blas_stack, const float4* __restrict__ rays, int n,
                                               void* __restrict__ out) {
  int *tl, *bl;
  lane_stacks(tlas_stack, blas_stack, tl, bl);
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (size_t)n) return;
  const float4 ra = rays[2 * i], rb = rays[2 * i + 1];
  const v3 o = mk3(ra.x, ra.y, ra.z), d = mk3(rb.x, rb.y, rb.z);
  const float t_max = ra.w;
  LocalCounters lc;                                               // never counted: queries leave urt_counters alone
  HitRec h; h.t = URT_INF; h.kid = 0; h.u = 0; h.v = 0;
  if (t_max > 0.0f) h = trace_ray<false, ANY>(S, o, d, t_max, tl, bl, lc);   // NaN / non-positive t_max: no t satisfies 0 < t < t_max
  if (ANY) {
    ((int32_t*)out)[i] = h.kind() != 0 ? 1 : 0;
    return;
  }
  const HitRecord r = hit_record(S, h, o, d);
  float4* o4 = (float4*)out + 3 * i;
  st_nt(o4, r.r0); st_nt(o4 + 1, r.r1); st_nt(o4 + 2, r.r2);
}

}  // namespace

namespace urtd {

hipError_t launch_query(const DevScene& S, LaneStackSize E, const float4* rays, int n, void* out, bool any_hit, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned int nb = (unsigned int)(((size_t)n + 255) / 256);
  const size_t lds = stack_lds_bytes(E, 256);
  if (hipError_t e = raise_lds_limit(any_hit ? (const void*)k_query<true> : (const void*)k_query<false>, lds)) return e;
  if (any_hit) hipLaunchKernelGGL(k_query<true>, dim3(nb), dim3(256), lds, st, S, E.tlas, E.blas, rays, n, out);
  else hipLaunchKernelGGL(k_query<false>, dim3(nb), dim3(256), lds, st, S, E.tlas, E.blas, rays, n, out);
  return hipGetLastError();
}

}  // namespace urtd
