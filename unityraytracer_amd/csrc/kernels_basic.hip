// kernels_basic.hip — the trace kernels without phase scheduling: kernel modes 0 (k_mega: one thread per pixel), 1 (k_generate / k_bounce:
// one launch per bounce over compacted path queues) and 2 (k_persist: persistent waves with path regeneration), and their launchers.
// Measured alternatives to the default kernel (kernels.hip k_sched) and bit-for-bit cross-checks of it (tests/test_gpu_parity.py):
// every device function they call is the one k_sched calls (frame_device.h).
#include "experiments.h"    // first: it looks at the -D switches before any default below is defined
#include "frame_device.h"
#include "launch_host.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// mode 0: per-pixel megakernel — the whole of CSMain (RS:431-469) in one thread.
// ---------------------------------------------------------------------------------------------------
template <bool COUNT>
__global__ __launch_bounds__(256) void k_mega(DevScene S, FrameParams P, float4* __restrict__ result, DevCounters* ctr) {
  int *tl, *bl;
  lane_stacks(P, tl, bl);
  LocalCounters lc;
  int x, y;
  if (tile_pixel(P, x, y)) {
    float px = (float)x, py = (float)y;
    float seed = P.seed;
    v3 avg = mk3(0, 0, 0);
    for (int i = 0; i < P.num_rays; i++) {
      v3 res = mk3(0, 0, 0);
      v3 o, d, energy = mk3(1, 1, 1);
      camera_ray<kPOffAfterScene>(P, x, y, seed, o, d);
      for (int k = 0; k < P.num_bounces; k++) {
        HitRec h = trace<COUNT>(S, o, d, tl, bl, lc);
        if (!shade<COUNT>(S, h, o, d, energy, res, seed, px, py, lc)) break;
      }
      avg = avg + res;
    }
    float n = (float)P.num_rays;
    st_nt(result + (size_t)y * P.width + x, make_float4(avg.x / n, avg.y / n, avg.z / n, 1.0f));
  }
  flush_counters<COUNT>(lc, ctr);
}

// ---------------------------------------------------------------------------------------------------
// mode 2 (default): persistent waves with path regeneration.
// A fixed grid of waves stays resident for the whole frame.  Every lane owns one path at a time; when
// enough lanes of a wave have finished their pixel (sky hit, energy gone, bounce limit) the wave
// ballots the dead lanes, takes that many new pixels from the frame's work counter with ONE atomic
// (prefix popcount gives each dead lane its slot) and starts their camera rays — so the 64 lanes stay
// busy through all bounces without per-bounce launches or path state round-trips through HBM.
// Pixels are handed out in tile order (64 consecutive slots = one 8x8 tile), so refills stay coherent.
// Per-pixel arithmetic is exactly CSMain's (RS:431-469); only the lane a pixel runs on changes.
// ---------------------------------------------------------------------------------------------------
template <bool COUNT>
__global__ __launch_bounds__(256) void k_persist(DevScene S, FrameParams P, float4* __restrict__ result, DevCounters* ctr,
                                                 unsigned int* __restrict__ next) {
  int *tl, *bl;
  lane_stacks(P, tl, bl);
  LocalCounters lc;
  const unsigned int ntiles = (unsigned int)(P.tiles_x * P.n_strips);
  WorkCursor wc; wc.shard = blockIdx.x & ((unsigned int)P.n_shards - 1u);
  bool alive = false, exhausted = false;
#ifdef URT_STAMPS
  unsigned long long t_start = wall_clock64(), t_exh = 0; unsigned int n_iter = 0, n_fetch = 0;
#endif
  int x = 0, y = 0, ray_i = 0, k = 0;
  float px = 0, py = 0, seed = 0;
  v3 o = mk3(0, 0, 0), d = mk3(0, 0, 1), energy = mk3(0, 0, 0), res = mk3(0, 0, 0), avg = mk3(0, 0, 0);
  for (;;) {
    unsigned long long dead = wballot(!alive);
    int ndead = __popcll(dead);
    if (!exhausted && ndead >= P.refill_min) {
      bool got = wave_fetch_pixels(P, dead, !alive, next, ntiles, wc, exhausted, x, y);
#ifdef URT_STAMPS
      n_fetch++; if (exhausted && !t_exh) t_exh = wall_clock64();
#endif
      if (got) {
        alive = true;
        px = (float)x; py = (float)y;
        seed = P.seed; ray_i = 0; k = 0;
        avg = mk3(0, 0, 0); res = mk3(0, 0, 0); energy = mk3(1, 1, 1);
        camera_ray<kPOffAfterScene>(P, x, y, seed, o, d);
      }
    }
    if (wballot(alive) == 0) {
      if (exhausted) break;
      continue;                       // every fetched slot fell outside the region: fetch again
    }
#ifdef URT_STAMPS
    n_iter++;
#endif
    if (alive) {
      HitRec h = trace<COUNT>(S, o, d, tl, bl, lc);
      bool cont = shade<COUNT>(S, h, o, d, energy, res, seed, px, py, lc);
      k++;
      if (!cont || k >= P.num_bounces) {            // RS:453,457-460
        avg = avg + res;                             // RS:464
        ray_i++;
        if (ray_i < P.num_rays) {                    // RS:444: next ray of this pixel, _Seed carries over
          res = mk3(0, 0, 0); energy = mk3(1, 1, 1); k = 0;
          camera_ray<kPOffAfterScene>(P, x, y, seed, o, d);
        } else {
          float n = (float)P.num_rays;
          st_nt(result + (size_t)y * P.width + x, make_float4(avg.x / n, avg.y / n, avg.z / n, 1.0f));   // RS:468
          alive = false;
        }
      }
    }
  }
#ifdef URT_STAMPS
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* st = (unsigned long long*)(next + kWorkShards * 32);
    size_t w = ((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4;
    st[w] = t_start; st[w + 1] = t_exh; st[w + 2] = wall_clock64(); st[w + 3] = ((unsigned long long)n_iter << 32) | n_fetch;
  }
#endif
  flush_counters<COUNT>(lc, ctr);
}

// ---------------------------------------------------------------------------------------------------
// mode 1: wavefront pipeline.  generate -> (bounce x num_bounces) per ray index, over compacted queues.
// ---------------------------------------------------------------------------------------------------
// Append the alive lanes of this wave to a queue: ballot, prefix popcount, one atomic per wave.
__device__ __forceinline__ int wave_append(bool alive, unsigned int* counter) {
  unsigned long long m = wballot(alive);
  if (m == 0) return -1;
  int lane = threadIdx.x & 63;
  int leader = __ffsll((long long)m) - 1;
  unsigned int base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned int)__popcll(m));
  base = __shfl(base, leader, 64);
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  return alive ? (int)(base + rank) : -1;
}

__global__ __launch_bounds__(256) void k_generate(FrameParams P, PathQueues Q, const float4* __restrict__ result,
                                                  int ray_index, DevCounters* ctr) {
  int x = 0, y = 0;
  bool ok = tile_pixel(P, x, y);
  float seed = P.seed;
  v3 o = mk3(0, 0, 0), d = mk3(0, 0, 0);
  if (ok) {
    if (ray_index > 0) seed = result[(size_t)y * P.width + x].w;
    camera_ray<0>(P, x, y, seed, o, d);
  }
  unsigned int* cnt = Q.counts + (size_t)ray_index * (P.num_bounces + 1);
  int slot = wave_append(ok, cnt);
  if (ok) {
    Q.s[0][0][slot] = make_float4(o.x, o.y, o.z, seed);
    Q.s[0][1][slot] = make_float4(d.x, d.y, d.z, as_float((y << 16) | x));
    Q.s[0][2][slot] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    Q.s[0][3][slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_bounce(DevScene S, FrameParams P, PathQueues Q, float4* __restrict__ result,
                                                int ray_index, int bounce, DevCounters* ctr) {
  int *tl, *bl;
  lane_stacks(P, tl, bl);
  LocalCounters lc;
  unsigned int* cnt = Q.counts + (size_t)ray_index * (P.num_bounces + 1) + bounce;
  unsigned int n_in = cnt[0];
  unsigned int gid = blockIdx.x * blockDim.x + threadIdx.x;
  int in = bounce & 1, out = in ^ 1;
  bool alive = false;
  v3 o, d, energy, res; float seed = 0; int pixel = 0;
  if (gid < n_in) {
    float4 s0 = Q.s[in][0][gid], s1 = Q.s[in][1][gid], s2 = Q.s[in][2][gid], s3 = Q.s[in][3][gid];
    o = xyz(s0); seed = s0.w; d = xyz(s1); pixel = as_int(s1.w); energy = xyz(s2); res = xyz(s3);
    float px = (float)(pixel & 0xffff), py = (float)((unsigned)pixel >> 16);
    HitRec h = trace<COUNT>(S, o, d, tl, bl, lc);
    alive = shade<COUNT>(S, h, o, d, energy, res, seed, px, py, lc);
    if (bounce == P.num_bounces - 1) alive = false;      // loop bound RS:453
    if (!alive) finish_path(P, result, pixel, ray_index, res, seed);
  }
  int slot = wave_append(alive, cnt + 1);
  if (alive) {
    Q.s[out][0][slot] = make_float4(o.x, o.y, o.z, seed);
    Q.s[out][1][slot] = make_float4(d.x, d.y, d.z, as_float(pixel));
    Q.s[out][2][slot] = make_float4(energy.x, energy.y, energy.z, 0.0f);
    Q.s[out][3][slot] = make_float4(res.x, res.y, res.z, 0.0f);
  }
  flush_counters<COUNT>(lc, ctr);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// host-side launchers (declared in kernels.h)
// ---------------------------------------------------------------------------------------------------
namespace urtd {

hipError_t launch_mega(const DevScene& S, const FrameParams& P, float4* result, DevCounters* ctr, bool count, hipStream_t st,
                       TraceLaunchRecord* rec) {
  int nb = blocks_for_tiles(P);
  if (nb == 0) return hipSuccess;
  return launch_traced(named(rec, "k_mega<%s>", tf(count)), count ? k_mega<true> : k_mega<false>, nb, P.block_threads, stack_lds_bytes(P), st,
                       S, P, result, ctr);
}

hipError_t launch_wavefront(const DevScene& S, const FrameParams& P, const PathQueues& Q, float4* result, DevCounters* ctr,
                            bool count, hipStream_t st, TraceLaunchRecord* rec) {
  int nb = blocks_for_tiles(P);
  if (nb == 0) return hipSuccess;
  size_t lds = stack_lds_bytes(P);
  size_t n_counts = (size_t)P.num_rays * (P.num_bounces + 1);
  hipError_t e = hipMemsetAsync(Q.counts, 0, n_counts * sizeof(unsigned int), st);
  if (e != hipSuccess) return e;
  auto bounce = count ? k_bounce<true> : k_bounce<false>;
  e = raise_lds_limit((const void*)bounce, lds);
  if (e != hipSuccess) return e;
  size_t npix = (size_t)P.region_w * 8 * P.n_strips;
  int bt = P.block_threads;
  int nbb = (int)((npix + bt - 1) / bt);
  for (int i = 0; i < P.num_rays; i++) {
    hipLaunchKernelGGL(k_generate, dim3(nb), dim3(bt), 0, st, P, Q, (const float4*)result, i, ctr);
    for (int k = 0; k < P.num_bounces; k++) hipLaunchKernelGGL(bounce, dim3(nbb), dim3(bt), lds, st, S, P, Q, result, i, k, ctr);
  }
  named(rec, "k_generate + k_bounce<%s> x %d", tf(count), P.num_rays * P.num_bounces);
  rec->n_blocks = nbb; rec->block_threads = bt; rec->lds_bytes = (int)lds;
  return hipGetLastError();
}

hipError_t launch_persist(const DevScene& S, const FrameParams& P, float4* result, DevCounters* ctr, unsigned int* next,
                          int n_blocks, bool count, hipStream_t st, TraceLaunchRecord* rec) {
  if (n_blocks <= 0) return hipSuccess;
  hipError_t e = reset_work_counters(next, st);
  if (e != hipSuccess) return e;
  return launch_traced(named(rec, "k_persist<%s>", tf(count)), count ? k_persist<true> : k_persist<false>, n_blocks, P.block_threads,
                       stack_lds_bytes(P), st, S, P, result, ctr, next);
}

}  // namespace urtd
