// radiance.hip — batched radiance queries against the prepared device scene (urt_radiance_query / urt_radiance_query_device,
// include/urt.h): "how much light arrives along this ray?" for arbitrary rays, and "what would a frame dispatched now write to this
// pixel?" for pixels of the bound camera.
//
// One query per lane, wave64, 256 threads per workgroup; per-lane LDS stacks (trace_device.h lane_stacks) sized from the prepared
// scene.  A query is the body of k_mega's pixel (RS:440-468): `samples` paths, one after the other on the same lane because the running
// seed chains them (RS:444), each of up to `bounces` iterations of Trace + Shade.  Trace is the frame kernels' (trace_device.h trace_ray,
// t_max = +inf) and so is Shade (shade_device.h), never counted.  Pixels mode builds its camera ray with the frame kernels' functions
// (camera_device.h), the uniforms arriving as a kernel-argument struct (as aov.hip's).
// Loads: three float4 per ray or one 8-byte record per pixel; stores: one non-temporal float4 per query.
//
// Two kernels run the same per-lane steps (query_begin / sample_begin / bounce_step) and differ only in which lane a query runs on:
//  * k_radiance: query i on thread i of the grid;
//  * k_radiance_persist: a resident grid whose lanes take the next query index from a work counter when theirs is finished (ballot of the
//    free lanes, ONE atomic per wave, prefix popcount — kernels_basic.hip k_persist's scheme), so a lane whose paths died on the sky does not
//    idle while a neighbour runs bounces x samples.  Its loop ends when the counter has passed n: no watchdog.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "camera_device.h"
#include "trace_device.h"
#include "sky_device.h"
#include "shade_device.h"
#include "radiance.h"
#include "launch_host.h"

namespace {

// free lanes of a wave that make k_radiance_persist go to the work counter (k_persist's refill_min default); once the counter has passed
// n the remaining paths simply run out
constexpr int kRefillMin = 16;

struct Lane {
  float px, py, seed;       // the "pixel" of rand() and the running seed
  v3 o0, d0;                // rays mode: the query's ray, every sample starts from it
  v3 o, d, energy, res, avg;
};

// Reads query i.  false: a pixel outside the Result (device form; the host form refuses it) — it gets (0, 0, 0, 0) and is not traced.
template <bool PIXELS>
__device__ __forceinline__ bool query_begin(const FrameUniforms& C, int width, int height, const void* __restrict__ in, size_t i, Lane& L) {
  L.avg = mk3(0, 0, 0);
  if (PIXELS) {
    const int2 p = ((const int2*)in)[i];
    L.px = (float)p.x; L.py = (float)p.y;
    L.seed = C.seed;                                             // RS:16: every pixel starts from the frame's _Seed
    return p.x >= 0 && p.x < width && p.y >= 0 && p.y < height;
  }
  const float4* r = (const float4*)in + 3 * i;
  const float4 ra = r[0], rb = r[1], rc = r[2];
  L.o0 = mk3(ra.x, ra.y, ra.z); L.seed = ra.w;
  L.d0 = mk3(rb.x, rb.y, rb.z);
  L.px = rc.x; L.py = rc.y;
  return true;
}

// The start of one sample: res = 0, energy = 1 and the sample's first ray — the query's own, or the camera ray of the pixel's next sample
template <bool PIXELS>
__device__ __forceinline__ void sample_begin(const FrameUniforms& C, int width, int height, Lane& L) {
  L.res = mk3(0, 0, 0); L.energy = mk3(1, 1, 1);
  if (PIXELS) {
    float u, v;
    jitter_uv(L.seed, L.px, L.py, C.pixel_off_x, C.pixel_off_y, width, height, u, v);
    camera_ray_uv(C.c2w, C.invp, u, v, L.o, L.d);
  } else {
    L.o = L.o0; L.d = L.d0;
  }
}

// One iteration of RS:453-460: Trace, then Shade; false = the path ends here
__device__ __forceinline__ bool bounce_step(const DevScene& S, Lane& L, int* tl, int* bl) {
  LocalCounters lc;                                              // never counted: queries leave urt_counters alone
  const HitRec h = trace_ray<false, false>(S, L.o, L.d, URT_INF, tl, bl, lc);
  return shade<false>(S, h, L.o, L.d, L.energy, L.res, L.seed, L.px, L.py, lc);
}

__device__ __forceinline__ void query_store(float4* __restrict__ out, size_t i, const Lane& L, int samples) {
  const float n = (float)samples;
  st_nt(out + i, make_float4(L.avg.x / n, L.avg.y / n, L.avg.z / n, 1.0f));   // RS:468
}

template <bool PIXELS>
__global__ __launch_bounds__(256) void k_radiance(DevScene S, int tlas_stack, int blas_stack, FrameUniforms C, int width, int height,
                                                  const void* __restrict__ in, int n, int samples, int bounces, float4* __restrict__ out) {
  int *tl, *bl;
  lane_stacks(tlas_stack, blas_stack, tl, bl);
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (size_t)n) return;
  Lane L;
  if (!query_begin<PIXELS>(C, width, height, in, i, L)) { st_nt(out + i, make_float4(0, 0, 0, 0)); return; }
  for (int s = 0; s < samples; s++) {
    sample_begin<PIXELS>(C, width, height, L);
    for (int k = 0; k < bounces; k++)
      if (!bounce_step(S, L, tl, bl)) break;
    L.avg = L.avg + L.res;                                       // RS:464
  }
  query_store(out, i, L, samples);
}

// bounces >= 1 (launch_radiance sends bounces == 0 to k_radiance: its paths have no step to schedule)
template <bool PIXELS>
__global__ __launch_bounds__(256) void k_radiance_persist(DevScene S, int tlas_stack, int blas_stack, FrameUniforms C, int width, int height,
                                                          const void* __restrict__ in, int n, int samples, int bounces,
                                                          float4* __restrict__ out, unsigned int* __restrict__ next) {
  const int lane = threadIdx.x & 63;
  int *tl, *bl;
  lane_stacks(tlas_stack, blas_stack, tl, bl);
  Lane L;
  L.px = L.py = L.seed = 0;
  L.o0 = L.o = mk3(0, 0, 0); L.d0 = L.d = mk3(0, 0, 1);
  L.energy = L.res = L.avg = mk3(0, 0, 0);
  bool alive = false, exhausted = false;                         // exhausted is wave-uniform: the counter has passed n
  unsigned int i = 0;
  int s = 0, k = 0;
  for (;;) {
    const unsigned long long dead = wballot(!alive);
    const unsigned int ndead = (unsigned int)__popcll(dead);
    if (!exhausted && ndead >= (unsigned int)kRefillMin) {
      unsigned int base = 0;
      if (lane == 0) base = atomicAdd(next, ndead);
      base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
      if (base + ndead >= (unsigned int)n) exhausted = true;     // the counter only grows, so this is final
      const unsigned int mine = base + (unsigned int)__popcll(dead & ((1ull << lane) - 1ull));
      if (!alive && mine < (unsigned int)n) {
        i = mine;
        if (query_begin<PIXELS>(C, width, height, in, i, L)) {
          alive = true; s = 0; k = 0;
          sample_begin<PIXELS>(C, width, height, L);
        } else {
          st_nt(out + i, make_float4(0, 0, 0, 0));
        }
      }
    }
    if (wballot(alive) == 0) {
      if (exhausted) break;
      continue;                                                  // every index drawn was an out-of-range pixel: draw again
    }
    if (alive) {
      const bool cont = bounce_step(S, L, tl, bl);
      k++;
      if (!cont || k >= bounces) {
        L.avg = L.avg + L.res;                                   // RS:464
        s++;
        if (s < samples) { k = 0; sample_begin<PIXELS>(C, width, height, L); }  // RS:444: the next sample, the seed carries over
        else { query_store(out, i, L, samples); alive = false; }
      }
    }
  }
}

template <bool PIXELS>
hipError_t launch_t(const DevScene& S, LaneStackSize E, const FrameUniforms& C, const RadianceBatch& B, hipStream_t st) {
  const size_t lds = stack_lds_bytes(E, 256);
  const bool persist = B.work_counter != nullptr && B.bounces > 0 && B.n_cus > 0;
  const void* fn = persist ? (const void*)k_radiance_persist<PIXELS> : (const void*)k_radiance<PIXELS>;
  if (hipError_t e = raise_lds_limit(fn, lds)) return e;
  const unsigned int all = (unsigned int)(((size_t)B.n + 255) / 256);
  if (persist) {
    hipError_t e = hipMemsetAsync(B.work_counter, 0, sizeof(unsigned int), st);
    if (e != hipSuccess) return e;
    int per_cu = 0;                                              // the resident grid: what fits the chip at once (registers, LDS)
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds);
    if (e != hipSuccess) return e;
    const unsigned int fit = (unsigned int)B.n_cus * (unsigned int)(per_cu > 0 ? per_cu : 1);
    const unsigned int nb = all < fit ? all : fit;
    hipLaunchKernelGGL(k_radiance_persist<PIXELS>, dim3(nb), dim3(256), lds, st, S, E.tlas, E.blas, C, B.width, B.height, B.in, B.n, B.samples,
                       B.bounces, B.out, B.work_counter);
  } else {
    hipLaunchKernelGGL(k_radiance<PIXELS>, dim3(all), dim3(256), lds, st, S, E.tlas, E.blas, C, B.width, B.height, B.in, B.n, B.samples, B.bounces,
                       B.out);
  }
  return hipGetLastError();
}

}  // namespace

namespace urtd {

hipError_t launch_radiance(const DevScene& S, LaneStackSize E, const FrameUniforms& C, const RadianceBatch& B, hipStream_t st) {
  if (B.n <= 0) return hipSuccess;
  return B.pixels ? launch_t<true>(S, E, C, B, st) : launch_t<false>(S, E, C, B, st);
}

}  // namespace urtd
