// kernels_pool.hip — kernel mode 4 (k_pool): persistent waves over a pool of paths kept in LDS, and its launcher.  A measured alternative
// to the default kernel (kernels.hip k_sched) and a bit-for-bit cross-check of it (tests/test_gpu_parity.py).
#include "experiments.h"    // first: it looks at the -D switches before any default below is defined
#include "front_device.h"     // trace_front (and frame_device.h)
#include "launch_host.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// mode 4: persistent waves over a POOL of paths (K x 64 path slots per wave, state in LDS).
// Measured on mode 3 (profiles/README.md): a wave that owns exactly 64 paths runs its triangle-BVH phase with 16-20 active
// lanes and its SHADE phase with ~30 — the paths of one wave are simply spread over the phases.  Every VALU instruction
// costs 4 cycles whatever the number of active lanes, and the kernel is ~45 % VALU-issue bound, so idle lanes are the cost.
// Here a wave owns NP = 64*K paths whose state (24 words, SoA [field][slot]) lives in LDS.  Each trip the wave takes a census
// of the slot states, elects ONE phase, compacts up to 64 slots that are in that phase onto its lanes (ballot + prefix
// popcount), loads what that phase needs, runs it, and stores the state back:
//     FREE -> FRONT -> BLAS -> RESUME -> ... -> SHADE -> FRONT | FREE
// The triangle-BVH phase keeps its 64 lanes fed from the list of waiting BLAS slots while it runs (a lane whose ray has
// finished retires it and takes the next one), and yields when few lanes are left; a suspended traversal stays PINNED to
// its lane, because its stack is the lane's ([entry][lane] in LDS), and resumes there.
// Per-pixel arithmetic and operation order are those of modes 0-3 (same device functions): pixels are bit-identical.
// ---------------------------------------------------------------------------------------------------
enum : int { PS_FREE = 0, PS_FRONT = 1, PS_RESUME = 2, PS_BLAS = 3, PS_PINNED = 4, PS_SHADE = 5 };
enum : int { F_PIX = 0, F_K, F_RAYI, F_SEED, F_OX, F_OY, F_OZ, F_DX, F_DY, F_DZ, F_EX, F_EY, F_EZ, F_RX, F_RY, F_RZ,
             F_T, F_KINDID, F_U, F_V, F_CHECK, F_CUR, F_SP, F_BESTI, F_COUNT1,      // _numRays == 1: 24 words per path
             F_AX = F_COUNT1, F_AY, F_AZ, F_COUNTN };                                // + resultAverage when _numRays > 1

// Slots whose state is in [lo, hi], in slot order: list[] receives all of them (`total`), lane L gets the L-th or -1.
template <int K>
__device__ __forceinline__ int pool_select(const int* stt, int* list, int lo, int hi, int& total) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0;
#pragma unroll
  for (int j = 0; j < K; j++) {
    int slot = j * 64 + lane;
    int v = stt[slot];
    bool m = v >= lo && v <= hi;
    unsigned long long b = wballot(m);
    if (m) list[base + __popcll(b & below)] = slot;
    base += __popcll(b);
  }
  total = base;
  __syncthreads();                 // one wave per workgroup: orders the LDS writes above before the reads below
  return lane < total ? list[lane] : -1;
}

template <bool COUNT, int K>
__global__ __launch_bounds__(64) void k_pool(DevScene S, FrameParams P, float4* __restrict__ result, DevCounters* ctr,
                                             unsigned int* __restrict__ next) {
  constexpr int NP = 64 * K;
  extern __shared__ int lds[];
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int* bl = lds + lane;                                // triangle-BVH stack of this LANE, entry e at bl[e * 64]
  int* pin = lds + P.blas_stack * 64;                  // [64] slot whose suspended traversal owns the lane's stack, or -1
  int* list = pin + 64;                                // [NP] compaction scratch
  int* stt = list + NP;                                // [NP] slot state
  int* pf = stt + NP;                                  // [fields][NP] path state
  const bool multi = P.num_rays > 1;
  int* tls = pf + (multi ? F_COUNTN : F_COUNT1) * NP;  // [tlas_stack][NP] object-level stack of each SLOT
#define PF(field, slot) pf[(field) * NP + (slot)]
#define PFf(field, slot) as_float(pf[(field) * NP + (slot)])
#define PFset(field, slot, val) pf[(field) * NP + (slot)] = as_int(val)
  pin[lane] = -1;
#pragma unroll
  for (int j = 0; j < K; j++) stt[j * 64 + lane] = PS_FREE;
  LocalCounters lc;
  const unsigned int ntiles = (unsigned int)(P.tiles_x * P.n_strips);
  WorkCursor wc; wc.shard = blockIdx.x & ((unsigned int)P.n_shards - 1u);
  bool exhausted = false, watchdog = false;
  unsigned int wave_iters = 0;
#ifdef URT_STAMPS
  unsigned long long ph_t[4] = {0, 0, 0, 0}, ph_lanes[5] = {0, 0, 0, 0, 0}, ph_trips[5] = {0, 0, 0, 0, 0};   // FRONT, BLAS, SHADE, blas inner, refill
  unsigned long long t_begin = wall_clock64(), t_dry = 0;
#endif

  for (;;) {
    if (watchdog) break;
#ifdef URT_STAMPS
    if (exhausted && !t_dry) t_dry = wall_clock64();
#endif
    __syncthreads();                                   // slot states written by other lanes during the last trip
    int nFree = 0, nFront = 0, nNew = 0, nPin = 0, nShade = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
      int v = stt[j * 64 + lane];
      nFree += __popcll(wballot(v == PS_FREE));
      nFront += __popcll(wballot(v == PS_FRONT || v == PS_RESUME));
      nNew += __popcll(wballot(v == PS_BLAS));
      nPin += __popcll(wballot(v == PS_PINNED));
      nShade += __popcll(wballot(v == PS_SHADE));
    }
    if (++wave_iters > P.sched_trips) { watchdog = true; break; }   // an exit every wave reaches, whatever the data
    const int busy = nFront + nNew + nPin + nShade;
    // ---- phase election ----
    // The triangle-BVH phase is the expensive one (hundreds of dependent steps per quantum, each costing the same whether
    // 8 or 64 lanes take part), so it waits until `blas_min` rays are queued for it; meanwhile the cheap phases run whenever
    // they have `pool_other_min` lanes of work, and free slots are refilled with new pixels.  Only when nothing reaches its
    // threshold does the fullest phase run.
    const int nB = nNew + nPin;
    const bool can_fetch = !exhausted && nFree > 0;
    int phase;
    if (nB >= P.blas_min) phase = PS_BLAS;
    else if (can_fetch && nFree >= P.refill_min) phase = PS_FREE;
    else if (nShade >= P.pool_other_min && nShade >= nFront) phase = PS_SHADE;
    else if (nFront >= P.pool_other_min) phase = PS_FRONT;
    else if (nShade >= P.pool_other_min) phase = PS_SHADE;
    else if (can_fetch) phase = PS_FREE;
    else if (busy == 0) break;                           // nothing in the pool and no work left to fetch
    else if (nB >= nShade && nB >= nFront) phase = PS_BLAS;
    else if (nShade >= nFront) phase = PS_SHADE;
    else phase = PS_FRONT;

    if (phase == PS_FREE) {
      // ---- new pixels into free slots (one atomic per refill) ----
      int total;
      int mine = pool_select<K>(stt, list, PS_FREE, PS_FREE, total);
#ifdef URT_STAMPS
      ph_trips[4]++; ph_lanes[4] += (unsigned long long)min(total, 64);
#endif
      int x = 0, y = 0;
      if (wave_fetch_pixels(P, wballot(mine >= 0), mine >= 0, next, ntiles, wc, exhausted, x, y)) {
        float seed = P.seed;
        v3 o, d;
        camera_ray<kPOffAfterScene>(P, x, y, seed, o, d);
        PF(F_PIX, mine) = x | (y << 16); PF(F_K, mine) = 0; PF(F_RAYI, mine) = 0; PFset(F_SEED, mine, seed);
        PFset(F_OX, mine, o.x); PFset(F_OY, mine, o.y); PFset(F_OZ, mine, o.z);
        PFset(F_DX, mine, d.x); PFset(F_DY, mine, d.y); PFset(F_DZ, mine, d.z);
        PFset(F_EX, mine, 1.0f); PFset(F_EY, mine, 1.0f); PFset(F_EZ, mine, 1.0f);
        PFset(F_RX, mine, 0.0f); PFset(F_RY, mine, 0.0f); PFset(F_RZ, mine, 0.0f);
        if (multi) { PFset(F_AX, mine, 0.0f); PFset(F_AY, mine, 0.0f); PFset(F_AZ, mine, 0.0f); }
        stt[mine] = PS_FRONT;
      }
      continue;
    }
#ifdef URT_STAMPS
    unsigned long long t_ph = wall_clock64();
    int ph_id = phase == PS_FRONT ? 0 : phase == PS_BLAS ? 1 : 2;
    ph_lanes[ph_id] += (unsigned long long)min(64, phase == PS_FRONT ? nFront : phase == PS_BLAS ? nB : nShade);
    ph_trips[ph_id]++;
#endif

    if (phase == PS_FRONT) {
      // ---------------- FRONT / RESUME: Trace() up to the next triangle-BVH visit (RS:364-383) ----------------
      int total;
      int mine = pool_select<K>(stt, list, PS_FRONT, PS_RESUME, total);
      if (mine >= 0) {
        bool fresh = stt[mine] == PS_FRONT;
        v3 o = mk3(PFf(F_OX, mine), PFf(F_OY, mine), PFf(F_OZ, mine)), d = mk3(PFf(F_DX, mine), PFf(F_DY, mine), PFf(F_DZ, mine));
        HitRec best; best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
        int check = 0; bool seen = false;
        if (!fresh) {
          int ki = PF(F_KINDID, mine), cs = PF(F_CHECK, mine);
          best.t = PFf(F_T, mine); best.kid = ki; best.u = PFf(F_U, mine); best.v = PFf(F_V, mine);
          check = cs >> 1; seen = (cs & 1) != 0;
        }
        int32_t cur = kBlasDone;
        bool need = trace_front<COUNT>(S, fresh, o, d, best, check, seen, tls + mine, NP, cur, lc);
        PFset(F_T, mine, best.t); PF(F_KINDID, mine) = best.kid; PFset(F_U, mine, best.u); PFset(F_V, mine, best.v);
        PF(F_CHECK, mine) = (check << 1) | (seen ? 1 : 0);
        if (need) { PF(F_CUR, mine) = cur; PF(F_SP, mine) = 0; PF(F_BESTI, mine) = -1; stt[mine] = PS_BLAS; }
        else stt[mine] = PS_SHADE;
      }
    } else if (phase == PS_BLAS) {
      // ---------------- BLAS: triangle BVH of one MeshObject per ray; lanes are re-fed from the waiting list ----------------
      int total;
      (void)pool_select<K>(stt, list, PS_BLAS, PS_BLAS, total);     // list[0, total) = the waiting rays, in slot order
      int taken = 0;
      int mys = pin[lane];                                          // a suspended traversal resumes on the lane that holds its stack
      const int n0 = min(64, nB);
      const int exit_below = (nShade + nFront > 0 || can_fetch) ? min(P.blas_exit, n0) : 1;
      v3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
      HitRec best; best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
      int32_t cur = kBlasDone; int sp = 0, best_i = -1;
      bool load = mys >= 0, first = true;
      BlasRay R = blas_ray(o, d);
      unsigned long long steps = 0;
      const unsigned long long step_cap = (unsigned long long)P.watchdog_steps * 64ull;   // between two re-feeds
      for (;;) {
        unsigned long long mA = wballot(mys >= 0);
        int nA = __popcll(mA);
        if (taken < total && (first || 64 - nA >= P.pool_inloop || nA < exit_below)) {     // feed the idle lanes
          int r = __popcll(~mA & below);
          if (mys < 0 && taken + r < total) { mys = list[taken + r]; load = true; }
          taken = min(total, taken + 64 - nA);
          steps = 0;
        }
        first = false;
        if (load) {
          int ki = PF(F_KINDID, mys);
          o = mk3(PFf(F_OX, mys), PFf(F_OY, mys), PFf(F_OZ, mys)); d = mk3(PFf(F_DX, mys), PFf(F_DY, mys), PFf(F_DZ, mys));
          best.t = PFf(F_T, mys); best.kid = ki; best.u = PFf(F_U, mys); best.v = PFf(F_V, mys);
          cur = PF(F_CUR, mys); sp = PF(F_SP, mys); best_i = PF(F_BESTI, mys);
          R = blas_ray(o, d);
          load = false;
        }
        mA = wballot(mys >= 0);
        nA = __popcll(mA);
        if (nA < exit_below) break;
        if (++steps > step_cap) { watchdog = true; break; }
#ifdef URT_STAMPS
        ph_trips[3]++; ph_lanes[3] += (unsigned long long)nA;
#endif
        // majority vote: this trip runs EITHER the interior-node step OR the leaf step (see mode 3)
        bool active = mys >= 0;
        bool interior = active && cur >= 0;
        int nI = __popcll(wballot(interior));
        if (nI >= nA - nI) {
          if (interior) cur = blas_node_step<COUNT>(S, cur, R, best.t, bl, sp, lc);
        } else if (active && !interior) {
          test_leaf<COUNT>(S, cur, o, d, best, best_i, lc);
          cur = blas_pop(bl, sp);
        }
        if (active && cur == kBlasDone) {                              // ray finished: back to the object-level walk (RS:323-325)
          PFset(F_T, mys, best.t); PF(F_KINDID, mys) = best.kid; PFset(F_U, mys, best.u); PFset(F_V, mys, best.v);
          stt[mys] = ((PF(F_CHECK, mys) >> 1) == 0 && S.n_spheres == 0) ? PS_SHADE : PS_RESUME;   // nothing of Trace() left: shade next
          pin[lane] = -1;
          mys = -1;
        }
      }
      if (mys >= 0) {                                                  // yield: the traversal stays pinned to this lane
        PFset(F_T, mys, best.t); PF(F_KINDID, mys) = best.kid; PFset(F_U, mys, best.u); PFset(F_V, mys, best.v);
        PF(F_CUR, mys) = cur; PF(F_SP, mys) = sp; PF(F_BESTI, mys) = best_i;
        stt[mys] = PS_PINNED;
        pin[lane] = mys;
      }
    } else {
      // ---------------- SHADE + bookkeeping of CSMain's loops (RS:444-468) ----------------
      int total;
      int mine = pool_select<K>(stt, list, PS_SHADE, PS_SHADE, total);
      if (mine >= 0) {
        int pix = PF(F_PIX, mine), k = PF(F_K, mine), ray_i = PF(F_RAYI, mine), ki = PF(F_KINDID, mine);
        int x = pix & 0xffff, y = (int)((unsigned)pix >> 16);
        float px = (float)x, py = (float)y, seed = PFf(F_SEED, mine);
        v3 o = mk3(PFf(F_OX, mine), PFf(F_OY, mine), PFf(F_OZ, mine)), d = mk3(PFf(F_DX, mine), PFf(F_DY, mine), PFf(F_DZ, mine));
        v3 energy = mk3(PFf(F_EX, mine), PFf(F_EY, mine), PFf(F_EZ, mine)), res = mk3(PFf(F_RX, mine), PFf(F_RY, mine), PFf(F_RZ, mine));
        HitRec best; best.t = PFf(F_T, mine); best.kid = ki; best.u = PFf(F_U, mine); best.v = PFf(F_V, mine);
        bool cont = shade<COUNT>(S, best, o, d, energy, res, seed, px, py, lc);
        k++;
        int nst = PS_FRONT;
        if (!cont || k >= P.num_bounces) {
          v3 avg = multi ? mk3(PFf(F_AX, mine), PFf(F_AY, mine), PFf(F_AZ, mine)) : mk3(0, 0, 0);
          avg = avg + res;
          ray_i++;
          if (ray_i < P.num_rays) {
            res = mk3(0, 0, 0); energy = mk3(1, 1, 1); k = 0;
            camera_ray<kPOffAfterScene>(P, x, y, seed, o, d);
            if (multi) { PFset(F_AX, mine, avg.x); PFset(F_AY, mine, avg.y); PFset(F_AZ, mine, avg.z); }
          } else {
            float n = (float)P.num_rays;
            st_nt(result + (size_t)y * P.width + x, make_float4(avg.x / n, avg.y / n, avg.z / n, 1.0f));
            nst = PS_FREE;
          }
        }
        if (nst != PS_FREE) {
          PF(F_K, mine) = k; PF(F_RAYI, mine) = ray_i; PFset(F_SEED, mine, seed);
          PFset(F_OX, mine, o.x); PFset(F_OY, mine, o.y); PFset(F_OZ, mine, o.z);
          PFset(F_DX, mine, d.x); PFset(F_DY, mine, d.y); PFset(F_DZ, mine, d.z);
          PFset(F_EX, mine, energy.x); PFset(F_EY, mine, energy.y); PFset(F_EZ, mine, energy.z);
          PFset(F_RX, mine, res.x); PFset(F_RY, mine, res.y); PFset(F_RZ, mine, res.z);
        }
        stt[mine] = nst;
      }
    }
#ifdef URT_STAMPS
    ph_t[ph_id] += wall_clock64() - t_ph;
#endif
  }
#ifdef URT_STAMPS
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* sp_ = (unsigned long long*)(next + kWorkShards * 32);
    size_t w = (size_t)blockIdx.x * 32;
    for (int q = 0; q < 4; q++) { sp_[w + q] = ph_t[q]; sp_[w + 4 + q] = ph_lanes[q]; sp_[w + 8 + q] = ph_trips[q]; }
    sp_[w + 12] = t_begin; sp_[w + 13] = wall_clock64(); sp_[w + 14] = t_dry; sp_[w + 15] = 0;
    sp_[w + 16] = ph_trips[4]; sp_[w + 17] = ph_lanes[4]; sp_[w + 18] = wave_iters;
  }
#endif
#undef PF
#undef PFf
#undef PFset
  if (watchdog && (threadIdx.x & 63) == 0) report_watchdog(P, ctr + (blockIdx.x & (kCounterShards - 1)));
  flush_counters<COUNT>(lc, ctr);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// host-side launchers (declared in kernels.h)
// ---------------------------------------------------------------------------------------------------
namespace urtd {

size_t pool_lds_bytes(const FrameParams& P, int k) {
  size_t np = (size_t)64 * (size_t)k;
  size_t fields = P.num_rays > 1 ? F_COUNTN : F_COUNT1;
  return ((size_t)P.blas_stack * 64 + 64 + np + np + fields * np + (size_t)P.tlas_stack * np) * sizeof(int);
}

using PoolKernel = void (*)(DevScene, FrameParams, float4*, DevCounters*, unsigned int*);
static PoolKernel pool_kernel(bool count, int k) {
  switch (k) {
    case 1: return count ? k_pool<true, 1> : k_pool<false, 1>;
    case 2: return count ? k_pool<true, 2> : k_pool<false, 2>;
    case 3: return count ? k_pool<true, 3> : k_pool<false, 3>;
    default: return count ? k_pool<true, 4> : k_pool<false, 4>;
  }
}

hipError_t launch_pool(const DevScene& S, const FrameParams& P, float4* result, DevCounters* ctr, unsigned int* next,
                       int n_blocks, int k, bool count, hipStream_t st, TraceLaunchRecord* rec) {
  if (n_blocks <= 0) return hipSuccess;
  if (P.width > 65535 || P.height > 65535 || k < 1 || k > 4) return hipErrorInvalidValue;   // pixel packed as y << 16 | x
  hipError_t e = reset_work_counters(next, st);
  if (e != hipSuccess) return e;
  return launch_traced(named(rec, "k_pool<%s, %d>", tf(count), k), pool_kernel(count, k), n_blocks, 64, pool_lds_bytes(P, k), st,
                       S, P, result, ctr, next);
}

}  // namespace urtd
