// aov.hip — per-pixel first-hit feature buffers ("arbitrary output variables": hit, normal, albedo, id) of the bound camera
// (urt_render_aov, include/urt.h).
//
// One camera ray per lane, wave64.  A wave covers one 8 x 8 pixel tile and a 256-thread workgroup a 16 x 16 block, so the rays of a wave
// leave the camera in a narrow cone and walk the same BVH nodes (the frame kernels' tiles are 8 x 8 for the same reason).  Per-lane LDS
// stacks laid out [entry][lane] as k_query's, sized from the prepared scene.  The camera ray is CreateCameraRay RS:142-153 with either
// the pixel centre or the uv of a frame's first sample (RS:448-449, bit-identical to frame_device.h camera_ray); the trace is
// query_trace<false> with t_max = +inf, i.e. exactly what urt_ray_query and the frame kernels' Trace return for that ray.
// Stores: one non-temporal float4 per pixel into each target that is present; an absent target costs nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "trace_device.h"
#include "sky_device.h"
#include "query_device.h"
#include "aov.h"

namespace {

__global__ __launch_bounds__(256) void k_aov(DevScene S, const float4* __restrict__ albedo_tab, int tlas_stack, int blas_stack, AovCamera C,
                                             AovTargets T) {
  extern __shared__ int lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int* tl = lds + wave * (tlas_stack + blas_stack) * 64 + lane;
  int* bl = tl + tlas_stack * 64;
  // workgroup = 16 x 16 pixels, wave = the 8 x 8 tile (wave & 1, wave >> 1) of it, lane = (lane & 7, lane >> 3) of the tile
  const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= T.width || y >= T.height) return;                     // partial tiles at the right and top edges
  const size_t pix = (size_t)y * (size_t)T.width + (size_t)x;

  // CreateCameraRay RS:142-153
  const float px = (float)x, py = (float)y;
  float u, v;
  if (C.frame_ray) {                                             // RS:448-449, sample 0 of a frame dispatched now (frame_device.h camera_ray)
    float seed = C.seed;
    float r0 = rand_next(seed, px, py);
    float r1 = rand_next(seed, px, py);
    u = (px + r0 + C.pixel_off_x) / (float)T.width * 2.0f - 1.0f;
    v = (py + r1 + C.pixel_off_y) / (float)T.height * 2.0f - 1.0f;
  } else {
    u = (px + 0.5f) / (float)T.width * 2.0f - 1.0f;
    v = (py + 0.5f) / (float)T.height * 2.0f - 1.0f;
  }
  const v3 o = mul_m4(C.c2w, 0.0f, 0.0f, 0.0f, 1.0f);
  v3 dir = mul_m4(C.invp, u, v, 0.0f, 1.0f);
  dir = mul_m4(C.c2w, dir.x, dir.y, dir.z, 0.0f);
  const v3 d = normalize(dir);

  const HitRec h = query_trace<false>(S, o, d, URT_INF, tl, bl);
  const HitRecord r = hit_record(S, h, o, d);                    // the urt_RayHit record urt_ray_query returns for this ray
  if (T.hit) st_nt(T.hit + pix, make_float4(r.r0.y, r.r0.z, r.r0.w, r.r0.x));                  // a miss: (0, 0, 0, +inf)
  if (T.normal) st_nt(T.normal + pix, make_float4(r.r1.x, r.r1.y, r.r1.z, (float)h.kind()));   // a miss: (0, 0, 0, 0)
  if (T.id) st_nt(T.id + pix, r.r2);                                                            // a miss: (-1, -1, 0, 0)
  if (T.albedo) {
    float4 a;
    if (h.kind() != 0) {
      // the material table's order (shade_device.h shade_surface): spheres, then MeshObjects, then the ground plane
      const int object = as_int(r.r2.x);
      a = albedo_tab[h.kind() == 1 ? S.n_spheres + S.n_meshes : h.kind() == 2 ? object : S.n_spheres + object];
    } else {
      const v3 s = sky_radiance(S, d);                           // what Shade returns for the miss (RS:420-427)
      a = make_float4(s.x, s.y, s.z, 0);
    }
    st_nt(T.albedo + pix, a);
  }
}

}  // namespace

namespace urtd {

hipError_t launch_aov(const DevScene& S, const float4* albedo, int tlas_stack, int blas_stack, const AovCamera& C, const AovTargets& T,
                      hipStream_t st) {
  if (T.width <= 0 || T.height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((T.width + 15) / 16), (unsigned int)((T.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  const size_t lds = (size_t)(tlas_stack + blas_stack) * 256 * sizeof(int);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_aov, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_aov, grid, dim3(256), lds, st, S, albedo, tlas_stack, blas_stack, C, T);
  return hipGetLastError();
}

}  // namespace urtd
