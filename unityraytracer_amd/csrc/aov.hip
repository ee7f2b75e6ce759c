// aov.hip — per-pixel first-hit feature buffers ("arbitrary output variables": hit, normal, albedo, id) of the bound camera
// (urt_render_aov, include/urt.h).
//
// One camera ray per lane, wave64.  A wave covers one 8 x 8 pixel tile and a 256-thread workgroup a 16 x 16 block, so the rays of a wave
// leave the camera in a narrow cone and walk the same BVH nodes (the frame kernels' tiles are 8 x 8 for the same reason).  Per-lane LDS
// stacks (trace_device.h lane_stacks) sized from the prepared scene.  The camera ray is the frame kernels' (camera_device.h) through
// either the pixel centre or the uv of a frame's first sample; the trace is trace_ray with t_max = +inf, the function urt_ray_query and
// the frame kernels' Trace call for that ray.
// Stores: one non-temporal float4 per pixel into each target that is present; an absent target costs nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "camera_device.h"
#include "trace_device.h"
#include "sky_device.h"
#include "query_device.h"
#include "aov.h"
#include "launch_host.h"

namespace {

__global__ __launch_bounds__(256) void k_aov(DevScene S, const float4* __restrict__ albedo_tab, int tlas_stack, int blas_stack, FrameUniforms C,
                                             int frame_ray, AovTargets T) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int *tl, *bl;
  lane_stacks(tlas_stack, blas_stack, tl, bl);
  // workgroup = 16 x 16 pixels, wave = the 8 x 8 tile (wave & 1, wave >> 1) of it, lane = (lane & 7, lane >> 3) of the tile
  const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= T.width || y >= T.height) return;                     // partial tiles at the right and top edges
  const size_t pix = (size_t)y * (size_t)T.width + (size_t)x;

  const float px = (float)x, py = (float)y;
  float u, v;
  if (frame_ray) {                                               // sample 0 of a frame dispatched now
    float seed = C.seed;
    jitter_uv(seed, px, py, C.pixel_off_x, C.pixel_off_y, T.width, T.height, u, v);
  } else {
    u = axis_uv(px + 0.5f, T.width);
    v = axis_uv(py + 0.5f, T.height);
  }
  v3 o, d;
  camera_ray_uv(C.c2w, C.invp, u, v, o, d);

  LocalCounters lc;                                              // never counted: urt_render_aov leaves urt_counters alone
  const HitRec h = trace_ray<false, false>(S, o, d, URT_INF, tl, bl, lc);
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

hipError_t launch_aov(const DevScene& S, const float4* albedo, LaneStackSize E, const FrameUniforms& C, bool frame_ray, const AovTargets& T,
                      hipStream_t st) {
  if (T.width <= 0 || T.height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((T.width + 15) / 16), (unsigned int)((T.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  const size_t lds = stack_lds_bytes(E, 256);
  if (hipError_t e = raise_lds_limit((const void*)k_aov, lds)) return e;
  hipLaunchKernelGGL(k_aov, grid, dim3(256), lds, st, S, albedo, E.tlas, E.blas, C, frame_ray ? 1 : 0, T);
  return hipGetLastError();
}

}  // namespace urtd
