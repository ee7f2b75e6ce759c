// frame_device.h — the device functions every frame kernel uses, whatever its mode (kernels.hip, kernels_basic.hip, kernels_serve.hip,
// kernels_pool.hip): Trace() as one call, the camera ray, tile and work-counter hand-out, the counter flush, the watchdog report.
// Everything here is inlined into its kernels; a translation unit includes it after experiments.h and gets the common preamble with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "kernels.h"

using namespace urt;
using namespace urtd;

#include "camera_device.h"    // jitter_uv, camera_ray_uv: the camera ray of a pixel
#include "trace_device.h"     // HitRec, slab tests, triangle / sphere / leaf tests, triangle-BVH node steps, intersect_mesh, trace_ray, lane_stacks, st_nt
#include "sky_device.h"       // sample_sky, sky_radiance: the sky lookup of Shade's miss branch
#include "shade_device.h"     // sample_hemisphere, shade_surface, shade_sky, shade: Shade RS:386-428

namespace {

// Trace — RS:364-383 — of the frame kernels that trace one ray per lane (modes 0 - 2): trace_device.h trace_ray, unbounded
template <bool COUNT>
__device__ __forceinline__ HitRec trace(const DevScene& S, v3 o, v3 d, int* tl, int* bl, LocalCounters& lc) {
  return trace_ray<COUNT, false>(S, o, d, URT_INF, tl, bl, lc);
}

// Cold per-pixel uniforms (the two camera matrices, 128 B) are read from the kernel-argument segment AT USE through a
// laundered pointer instead of living in 32 SGPRs for the whole kernel: with them resident the register allocator spilled
// and re-loaded the hot BVH pointers inside the traversal loop (an s_load + s_waitcnt on every node step).
typedef const __attribute__((address_space(4))) float* kfloatp;
__device__ __forceinline__ kfloatp kernarg_floats(unsigned byte_offset) {
  const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  p += byte_offset;
  asm volatile("" : "+s"(p));                      // opaque to LICM: the loads below stay where they are written
  return (kfloatp)p;
}

// The camera ray of pixel (x, y), camera_device.h.  P_OFF = byte offset of the FrameParams argument in the kernarg segment.
template <unsigned P_OFF>
__device__ __forceinline__ void camera_ray(const FrameParams& P, int x, int y, float& seed, v3& o, v3& d) {
  float u, v;
  jitter_uv(seed, (float)x, (float)y, P.pixel_off_x, P.pixel_off_y, P.width, P.height, u, v);
  kfloatp c2w = kernarg_floats(P_OFF + (unsigned)__builtin_offsetof(FrameParams, c2w));
  kfloatp invp = kernarg_floats(P_OFF + (unsigned)__builtin_offsetof(FrameParams, invp));
  camera_ray_uv(c2w, invp, u, v, o, d);
}
// The same for a batched launch (modes 3, 5): the uniforms of the path's frame come from the launch's frame table in device
// memory, read with scalar loads (table pointer and frame index are wave-uniform).  `f` must be wave-uniform.
// A NEW pixel's two draws start from the frame's _Seed and _Seed + 0.5 in every lane, and the ray's origin is the same for the whole
// frame: the seed-only half of both draws (two constant divisions each) and the origin come from the table entry, where the host put
// them (frame_derived.h: the same urt_math.h functions on the same operands), and only rand_draw runs per lane.  The next ray of a
// pixel carries its own seed and draws as before.  -DURT_UNIFORM_REFILL=0 (an experiment build): everything per lane, as it was.
#ifndef URT_UNIFORM_REFILL
#define URT_UNIFORM_REFILL 1
#endif
__device__ __forceinline__ void camera_ray_frame(const FrameEntry* T, int f, const FrameParams& P, int x, int y, bool new_pixel, float& seed, v3& o, v3& d) {
  kfloatp q = (kfloatp)(unsigned long long)(T + __builtin_amdgcn_readfirstlane(f));
  float px = (float)x, py = (float)y;
  if (URT_UNIFORM_REFILL && new_pixel) {
    float r0 = rand_draw(q[36], px, py);
    float r1 = rand_draw(q[37], px, py);
    seed = (q[34] + 0.5f) + 0.5f;                  // the two steps of the two draws, not one add
    float u = axis_uv(px + r0 + q[32], P.width);
    float v = axis_uv(py + r1 + q[33], P.height);
    v3 dir = mul_m4_k(q + 16, u, v, 0.0f, 1.0f);   // camera_ray_uv with the origin read instead of computed
    dir = mul_m4_k(q, dir.x, dir.y, dir.z, 0.0f);
    o = mk3(q[38], q[39], q[40]);
    d = normalize(dir);
    return;
  }
  if (new_pixel) seed = q[34];                     // RS:16: every pixel starts from the frame's _Seed; it carries over between a pixel's rays (RS:444)
  float r0 = rand_next(seed, px, py);
  float r1 = rand_next(seed, px, py);
  float u = axis_uv(px + r0 + q[32], P.width);     // jitter_uv written out: called through it, the table entry's scalar loads land elsewhere and k_sched's bytes change
  float v = axis_uv(py + r1 + q[33], P.height);
  camera_ray_uv(q, q + 16, u, v, o, d);
}
static_assert(__builtin_offsetof(FrameUniforms, invp) == 64 && __builtin_offsetof(FrameUniforms, pixel_off_x) == 128 &&
              __builtin_offsetof(FrameUniforms, seed) == 136 && __builtin_offsetof(FrameEntry, d) == 144 && __builtin_offsetof(FrameDerived, a1) == 4 &&
              __builtin_offsetof(FrameDerived, origin) == 8 && sizeof(FrameEntry) == 164, "camera_ray_frame indexes the table as floats");

// Runs body(frame index as a wave-uniform value, lane predicate) once per distinct frame among the lanes of `pred` (almost
// always one: a wave's refill straddles two frames only at a frame boundary of the launch).
template <typename F>
__device__ __forceinline__ void for_each_frame(bool pred, int frame, F&& body) {
  unsigned long long todo = wballot(pred);
  while (todo) {
    int f = __builtin_amdgcn_readlane(frame, __builtin_ctzll(todo));
    bool mine = pred && frame == f;
    body(f, mine);
    todo &= ~wballot(mine);
  }
}

// kernels take (DevScene, FrameParams, ...) or (FrameParams, ...): by-value aggregates are laid out like C struct members
static constexpr unsigned kPOffAfterScene = (unsigned)((sizeof(DevScene) + alignof(FrameParams) - 1) / alignof(FrameParams) * alignof(FrameParams));

// tile -> pixel: one 8x8 tile per wave (the reference's [numthreads(8,8,1)] group, RS:431).
// Blocks are dealt round-robin to the 8 XCDs (b % 8 shares an XCD, each XCD has a private 4 MiB L2).
// xcd_run = G makes every XCD walk runs of G consecutive blocks (G * waves-per-block adjacent tiles):
// G = 1 is plain linear order, large G approaches one contiguous image band per XCD (best L2 locality,
// worst load balance: sky bands finish early).  Only speed depends on it, never results.
__device__ __forceinline__ bool tile_pixel(const FrameParams& P, int& x, int& y) {
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int b = blockIdx.x;
  int G = P.xcd_run;
  int sb = ((b / (8 * G)) * 8 + (b & 7)) * G + ((b >> 3) % G);
  int tile = sb * (blockDim.x >> 6) + wave;
  int ntiles = P.tiles_x * P.n_strips;
  if (tile >= ntiles) return false;
  int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
  x = tx * 8 + (lane & 7);
  y = (P.first_group_row + ty * P.row_stride) * 8 + (lane >> 3);
  return x < P.region_w && y < P.region_h;
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool COUNT>
__device__ __forceinline__ void flush_counters(const LocalCounters& lc, DevCounters* ctr) {
  // wave-reduce, then one atomic per wave and counter into one of kCounterShards slots: tens of
  // thousands of same-address atomics serialise at ~88/us on this chip, sharded ones do not.
  ctr += (blockIdx.x & (kCounterShards - 1));
  unsigned int r = wave_sum(lc.rays);
  unsigned int tn = 0, bn = 0, tt = 0, st = 0, ht = 0, hs = 0, hg = 0, hk = 0;
  if (COUNT) {
    tn = wave_sum(lc.tlas_nodes); bn = wave_sum(lc.blas_nodes); tt = wave_sum(lc.tri_tests); st = wave_sum(lc.sphere_tests);
    ht = wave_sum(lc.hit_tri); hs = wave_sum(lc.hit_sphere); hg = wave_sum(lc.hit_ground); hk = wave_sum(lc.hit_sky);
  }
  if ((threadIdx.x & 63) == 0) {
    if (r) atomicAdd(&ctr->rays, (unsigned long long)r);
    if (COUNT) {
      if (tn) atomicAdd(&ctr->tlas_nodes, (unsigned long long)tn);
      if (bn) atomicAdd(&ctr->blas_nodes, (unsigned long long)bn);
      if (tt) atomicAdd(&ctr->tri_tests, (unsigned long long)tt);
      if (st) atomicAdd(&ctr->sphere_tests, (unsigned long long)st);
      if (ht) atomicAdd(&ctr->hit_tri, (unsigned long long)ht);
      if (hs) atomicAdd(&ctr->hit_sphere, (unsigned long long)hs);
      if (hg) atomicAdd(&ctr->hit_ground, (unsigned long long)hg);
      if (hk) atomicAdd(&ctr->hit_sky, (unsigned long long)hk);
    }
  }
}

__device__ __forceinline__ void lane_stacks(const FrameParams& P, int*& tl, int*& bl) { lane_stacks(P.tlas_stack, P.blas_stack, tl, bl); }

// Work distribution of the persistent kernels.  The frame is a sequence of pixel slots in tile order (64 consecutive slots
// = one 8x8 tile).  One shared counter would be hit ~40,000 times per 1080p frame, and same-address atomics serialise at
// ~88/us on this chip — that alone cost 0.4 ms.  So the tiles are dealt round-robin to kWorkShards counters (tile t belongs
// to shard t % kWorkShards, each counter on its own 128-byte line); a wave draws from its home shard (its workgroup index)
// and moves on to the next shard when that one is dry.  All shards advance at a similar pace, so the frame is still swept
// roughly in natural order.
struct WorkCursor {
  unsigned int shard;       // shard this wave currently draws from
};
static_assert(kWorkShards == 64, "the dry-shard probe reads one counter per lane");

// Tiles are dealt to the shards in RUNS of G = P.xcd_run consecutive tiles (run r belongs to shard r % kWorkShards).  G = 1
// interleaves single tiles; a large G gives every shard contiguous image bands, and because workgroup b runs on XCD b % 8
// and starts on shard b % kWorkShards, each XCD's L2 then serves a few bands of the image instead of all of it.
__device__ __forceinline__ unsigned int shard_slots(unsigned int ntiles, unsigned int shard, unsigned int G, unsigned int NS) {   // slots owned by a shard
  unsigned int cycle = NS * G;
  unsigned int full = ntiles / cycle, rem = ntiles - full * cycle;
  unsigned int extra = rem > shard * G ? min(rem - shard * G, G) : 0u;
  return (full * G + extra) * 64u;
}
__device__ __forceinline__ unsigned int shard_tile(unsigned int shard, unsigned int q, unsigned int G, unsigned int NS) {   // q-th tile of a shard
  unsigned int run = q / G;
  return (run * NS + shard) * G + (q - run * G);
}

// slot -> pixel; false for slots that fall outside the dispatched region (ragged right/top edge)
__device__ __forceinline__ bool slot_pixel(const FrameParams& P, unsigned int tile, unsigned int l, int& x, int& y) {
  int ty = (int)tile / P.tiles_x, tx = (int)tile - ty * P.tiles_x;
  x = tx * 8 + (int)(l & 7u);
  y = (P.first_group_row + ty * P.row_stride) * 8 + (int)(l >> 3);
  return x < P.region_w && y < P.region_h;
}

// The wave takes popcount(want) slots with ONE atomic; each lane of `want` gets its own slot (prefix popcount).  Returns true
// and the pixel for lanes that received a valid one.  Sets `exhausted` when every shard is dry.
// Batched launches (mode 3): the work is the concatenation of the frames' tile sequences (ntiles = frames x tiles_per_frame,
// frame-major, so the launch sweeps frame 0 first); `frame` receives the frame a slot belongs to.
__device__ __forceinline__ bool wave_fetch_pixels(const FrameParams& P, unsigned long long want, bool mine, unsigned int* next,
                                                  unsigned int ntiles, WorkCursor& wc, bool& exhausted, int& x, int& y,
                                                  unsigned int tiles_per_frame = 0, int* frame = nullptr) {
  const int lane = threadIdx.x & 63;
  unsigned int n = (unsigned int)__popcll(want);
  const unsigned int G = (unsigned int)P.xcd_run, NS = (unsigned int)P.n_shards;
  unsigned int own = shard_slots(ntiles, wc.shard, G, NS);
  unsigned int base = 0;
  if (lane == 0) base = atomicAdd(next + wc.shard * 32u, n);
  base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);   // called by the whole wave: lane 0's value, and wave-uniform for the compiler (what hangs off it — shard moves, `exhausted` — stays in scalar registers)
  unsigned int shard = wc.shard;
  if (base + n >= own) {   // this shard is (now) dry: every lane looks at one counter, the wave moves to the next shard with work
    unsigned int seen = __hip_atomic_load(next + lane * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long avail = wballot((unsigned int)lane < NS && seen < shard_slots(ntiles, (unsigned int)lane, G, NS)) & ~(1ull << shard);
    if (!avail) {
      exhausted = true;    // counters only grow, so this is final
    } else {
      unsigned long long after = shard == 63u ? 0ull : avail & ~((2ull << shard) - 1ull);
      wc.shard = (unsigned int)__builtin_ctzll(after ? after : avail);
    }
  }
  unsigned int local = base + (unsigned int)__popcll(want & ((1ull << lane) - 1ull));
  if (!mine || local >= own) return false;
  unsigned int tile = shard_tile(shard, local >> 6, G, NS);
  if (frame) {
    const unsigned int FG = (unsigned int)P.frame_group;
    if (FG <= 1u) { unsigned int f = tile / tiles_per_frame; tile -= f * tiles_per_frame; *frame = (int)f; }
    else {
      // frames interleaved in groups of FG: the global sequence is run 0 of frames 0..FG-1, run 1 of frames 0..FG-1, ... — the same
      // tiles of consecutive frames (same pixels, other jitter and seeds) are traced back to back, while their BVH subtrees are hot
      unsigned int rg = tile / G, w = tile - rg * G;
      unsigned int runs_pf = (tiles_per_frame + G - 1u) / G, group_runs = runs_pf * FG;
      unsigned int grp = rg / group_runs, r = rg - grp * group_runs;
      unsigned int f = grp * FG + r % FG;
      tile = (r / FG) * G + w;
      *frame = (int)f;
      if (tile >= tiles_per_frame || f >= (unsigned int)P.n_frames) return false;
    }
    ntiles = tiles_per_frame;
  }
  if (P.tile_order == 1) tile = ntiles - 1u - tile;            // top strip first
  return slot_pixel(P, tile, local & 63u, x, y);
}

// ---- The hand-out per WORKGROUP (mode 3, P.handout > 0) ----
// wave_fetch_pixels parks the whole wave, live lanes too, on a device-scope atomic (~2.3 us) at every refill.  Here the waves of a
// workgroup share a RESERVATION in LDS instead: one 64-bit word that names a chunk of C = P.handout consecutive tiles of the workgroup's
// shard (C divides P.xcd_run, so a chunk lies inside one run and therefore inside one frame of an interleaved launch) and how many of its
// slots are handed out.  A refill takes its slots with a compare-and-swap on that word — an LDS round trip — and only the wave that
// drains a chunk goes to the shard's counter, for the whole next chunk: one device-scope atomic per C x 64 slots instead of one per refill.
// The word, low bit first:
//   used 11 | valid 11 | fetching 1 | exhausted 1 | first tile of the chunk inside its frame 24 | frame 7 | shard 6
// `valid` > `used` only between the install of a chunk and its drain, and no two chunks of a launch share (frame, first tile): a
// compare-and-swap that takes slots can never succeed on another chunk's word (no ABA).  Drained words may repeat (a dry shard, a padded
// chunk); the only transition out of them is the one that sets `fetching`, which is right for whoever wins it.
// Termination: nothing here waits for another wave.  The wave that set `fetching` depends on no one — it adds to the counter, maps the
// chunk and installs the word; `fetching` set means that wave is between those steps.  A wave that finds it set skips this refill and
// runs its live lanes; with none it goes round the scheduler loop (a short s_sleep first), which P.sched_trips bounds like every other
// trip.  A failed compare-and-swap means another wave's succeeded; it is retried a fixed number of times, then the refill is skipped.
static constexpr unsigned long long kRunFetching = 1ull << 22, kRunExhausted = 1ull << 23;
static constexpr int kRunCasTries = 8;

__device__ __forceinline__ unsigned long long wave_uniform64(unsigned long long v) {
  unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)v);
  unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long run_word(unsigned int shard, unsigned int frame, unsigned int tile0, unsigned int valid, bool exhausted) {
  return ((unsigned long long)shard << 55) | ((unsigned long long)frame << 48) | ((unsigned long long)tile0 << 24) | (exhausted ? kRunExhausted : 0ull) |
         ((unsigned long long)valid << 11);
}

// The wave that holds `fetching` takes the next chunk of the workgroup's shard from its counter and returns the word to install:
// wave_fetch_pixels' bookkeeping (dry-shard probe, move to the next shard, `exhausted`) and its slot -> (frame, tile) arithmetic, once
// per chunk and on wave-uniform values.
__device__ __forceinline__ unsigned long long wg_fetch_run(const FrameParams& P, unsigned int shard, unsigned int* next, unsigned int ntiles,
                                                           unsigned int tiles_per_frame) {
  const int lane = threadIdx.x & 63;
  const unsigned int G = (unsigned int)P.xcd_run, NS = (unsigned int)P.n_shards, C = (unsigned int)P.handout;
  const unsigned int own = shard_slots(ntiles, shard, G, NS);
  unsigned int base = 0;
  if (lane == 0) base = atomicAdd(next + shard * 32u, C * 64u);
  base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
  unsigned int nshard = shard;
  bool exh = false;
  if (base + C * 64u >= own) {   // this shard is (now) dry: every lane looks at one counter, the workgroup moves to the next shard with work
    unsigned int seen = __hip_atomic_load(next + lane * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long avail = wballot((unsigned int)lane < NS && seen < shard_slots(ntiles, (unsigned int)lane, G, NS)) & ~(1ull << shard);
    if (!avail) exh = true;      // counters only grow, so this is final (the chunk below, if any, is the workgroup's last)
    else {
      unsigned long long after = shard == 63u ? 0ull : avail & ~((2ull << shard) - 1ull);
      nshard = (unsigned int)__builtin_ctzll(after ? after : avail);
    }
  }
  unsigned int vt = 0, f = 0, t0 = 0;                 // tiles of the chunk that exist, its frame, its first tile there
  if (base < own) {
    const unsigned int q0 = base >> 6;                // (every add is C x 64: q0 is a multiple of C, and C divides G)
    vt = min(C, (own >> 6) - q0);
    unsigned int tile = shard_tile(shard, q0, G, NS);
    const unsigned int FG = (unsigned int)P.frame_group;
    if (FG <= 1u) { f = tile / tiles_per_frame; t0 = tile - f * tiles_per_frame; }   // frame after frame: a chunk may run on into the next frames (wg_fetch_pixels)
    else {                                            // frames interleaved in groups of FG, as in wave_fetch_pixels
      unsigned int rg, w, grp, r, q;
      const unsigned int runs_pf = (tiles_per_frame + G - 1u) / G, group_runs = runs_pf * FG;
      if ((G & (G - 1u)) == 0u) { rg = tile >> __builtin_ctz(G); w = tile & (G - 1u); } else { rg = tile / G; w = tile - rg * G; }
      grp = rg / group_runs; r = rg - grp * group_runs;
      if ((FG & (FG - 1u)) == 0u) { q = r >> __builtin_ctz(FG); f = grp * FG + (r & (FG - 1u)); } else { q = r / FG; f = grp * FG + (r - q * FG); }
      t0 = q * G + w;
      if (t0 >= tiles_per_frame || f >= (unsigned int)P.n_frames) { vt = 0; f = 0; t0 = 0; }   // padding of a frame's last run, of the last group
      else vt = min(vt, tiles_per_frame - t0);
    }
  }
  return run_word(nshard, f, t0, vt * 64u, exh);
}

// wave_fetch_pixels for a workgroup that shares a reservation `rs` (LDS): the same slots map to the same pixels, handed out in another
// order.  Lanes the chunk has no slot for stay dead this trip, except in the wave that fetches the next chunk: it takes the rest there.
__device__ __forceinline__ bool wg_fetch_pixels(const FrameParams& P, unsigned long long want, bool mine, unsigned int* next,
                                                unsigned int ntiles, unsigned long long* rs, bool& exhausted, int& x, int& y,
                                                unsigned int tiles_per_frame, int* frame, unsigned long long* n_adds = nullptr) {   // n_adds: -DURT_STAMPS, device-scope atomics issued
  const int lane = threadIdx.x & 63;
  const unsigned int n = (unsigned int)__popcll(want);
  const unsigned int rank = (unsigned int)__popcll(want & ((1ull << lane) - 1ull));
  unsigned int taken = 0;
  bool got = false;
  for (int round = 0; round < 2; round++) {
    unsigned long long s = 0;
    unsigned int k = 0, avail = 0;
    bool fetch = false;
    for (int tries = 0;; tries++) {
      if (tries == kRunCasTries) return got;
      s = wave_uniform64(__hip_atomic_load(rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      avail = ((unsigned int)(s >> 11) & 0x7ffu) - ((unsigned int)s & 0x7ffu);
      unsigned long long s2;
      if (avail) {
        k = min(n - taken, avail);
        fetch = k == avail && !(s & kRunExhausted);           // this wave drains the chunk: it fetches the next one
        s2 = (s + k) | (fetch ? kRunFetching : 0ull);
      } else if (s & kRunExhausted) { exhausted = true; return got; }
      else if (s & kRunFetching) { if (n == 64u) __builtin_amdgcn_s_sleep(2); return got; }   // another wave is fetching: no refill this trip
      else { k = 0; fetch = true; s2 = s | kRunFetching; }
      unsigned long long seen = s;
      if (lane == 0) __hip_atomic_compare_exchange_strong(rs, &seen, s2, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (wave_uniform64(seen) == s) break;
    }
#if URT_UNIFORM_REFILL
    // The k slots are consecutive slots of the chunk (k <= popcount(want) <= 64): they lie in at most two of its tiles.  Frame, tile order and the tile's pixel origin
    // (a division by tiles_x, the strip arithmetic) are worked out once per tile on wave-uniform values, in scalar registers; what is
    // left per lane is the slot's place inside its 8x8 tile and the region test.  slot_pixel's integers, tile by tile.
    if (k) {
      const unsigned int first = (unsigned int)s & 0x7ffu;
      const unsigned int idx = first + (rank - taken);
      const bool in = mine && rank >= taken && rank < taken + k;
      for (unsigned int t = first >> 6; t <= (first + k - 1u) >> 6; t++) {
        unsigned int tile = ((unsigned int)(s >> 24) & 0xffffffu) + t, f = (unsigned int)(s >> 48) & 0x7fu;
        if (tile >= tiles_per_frame) { unsigned int q = tile / tiles_per_frame; f += q; tile -= q * tiles_per_frame; }   // frame_group 1 only: the chunk runs on into the next frame
        if (P.tile_order == 1) tile = tiles_per_frame - 1u - tile;   // top strip first
        const int ty = (int)tile / P.tiles_x, tx = (int)tile - ty * P.tiles_x;
        const int x0 = tx * 8, y0 = (P.first_group_row + ty * P.row_stride) * 8;
        if (in && (idx >> 6) == t) {
          *frame = (int)f;
          x = x0 + (int)(idx & 7u);
          y = y0 + (int)((idx >> 3) & 7u);
          got = x < P.region_w && y < P.region_h;
        }
      }
    }
#else
    if (mine && rank >= taken && rank < taken + k) {
      const unsigned int idx = ((unsigned int)s & 0x7ffu) + (rank - taken);
      unsigned int tile = ((unsigned int)(s >> 24) & 0xffffffu) + (idx >> 6), f = (unsigned int)(s >> 48) & 0x7fu;
      if (tile >= tiles_per_frame) { unsigned int q = tile / tiles_per_frame; f += q; tile -= q * tiles_per_frame; }   // frame_group 1 only: the chunk runs on into the next frame
      *frame = (int)f;
      if (P.tile_order == 1) tile = tiles_per_frame - 1u - tile;   // top strip first
      got = slot_pixel(P, tile, idx & 63u, x, y);
    }
#endif
    taken += k;
    if (!fetch) { if (k == avail) exhausted = true; break; }   // (no fetch after a drain: it was the workgroup's last chunk)
    const unsigned long long ns = wg_fetch_run(P, (unsigned int)(s >> 55) & 63u, next, ntiles, tiles_per_frame);
    if (lane == 0) __hip_atomic_store(rs, ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (the only writer while `fetching` is set)
    if (n_adds) ++*n_adds;
    if (taken == n) break;
  }
  return got;
}

// Every persistent kernel leaves its scheduler loop after P.sched_trips trips per wave, whatever the data (a frame needs ~1e3-1e5;
// the host scales the cap with the launch: frames x rays x bounces, frame_batch.cpp).  A wave that leaves that way — or through the
// per-phase traversal cap — counts itself in DevCounters::watchdog and raises the host-visible flag: its pixels are missing.
__device__ __forceinline__ void report_watchdog(const FrameParams& P, DevCounters* shard) {
  atomicAdd(&shard->watchdog, 1ull);
  if (P.trip_flag) __hip_atomic_fetch_add(P.trip_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Path finished: fold its radiance into the pixel.  Result.xyz holds the running resultAverage
// (RS:441,464) and .w the running _Seed between the rays of one pixel; the last ray writes RS:468.
__device__ __forceinline__ void finish_path(const FrameParams& P, float4* result, int pixel, int ray_index, v3 res, float seed) {
  int x = pixel & 0xffff, y = (unsigned)pixel >> 16;
  size_t at = (size_t)y * P.width + x;
  v3 avg = res;
  if (ray_index > 0) { float4 prev = result[at]; avg = xyz(prev) + res; }
  if (ray_index == P.num_rays - 1) {
    float n = (float)P.num_rays;
    result[at] = make_float4(avg.x / n, avg.y / n, avg.z / n, 1.0f);
  } else {
    result[at] = make_float4(avg.x, avg.y, avg.z, seed);
  }
}

}  // namespace
