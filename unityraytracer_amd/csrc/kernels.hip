// kernels.hip — hand-written HIP kernels for gfx950 (MI355X, CDNA4): the path-tracing hot path of
// RemyMuj/UnityRayTracer re-designed for 64-wide wavefronts.
//
// Reference being replaced: Assets/Shaders/RayTraceShader.compute ("RS", kernel CSMain RS:431-469 and
// everything it calls) and Assets/Shaders/AdditionShader.shader ("AS", AS:9,39-41).
//
// This is not a translation of the HLSL:
//  * the reference intersects EVERY triangle of a mesh per ray (RS:243); here each MeshObject has a
//    triangle BVH over pre-transformed world-space triangles (v0, e1, e2 as float4 records), traversed
//    with a per-lane stack that lives in LDS ([entry][lane] layout: conflict-free, no scratch);
//  * the reference carries a 68-byte RayHit with the material through traversal (RS:36-41); here the
//    traversal carries (t, kind, id, u, v) and normals/material are fetched once per closest hit;
//  * the reference is one thread per pixel for all bounces; the default kernel here (k_sched, kernel_mode 3) keeps a
//    fixed grid of waves resident for the whole frame: a lane whose path has ended takes a new pixel from the frame's
//    sharded work counter (wave64 ballot + prefix popcount; the waves of a workgroup draw through a shared reservation in LDS), and the lanes of a wave are
//    scheduled by phase (object-level walk / triangle-BVH loop / shading) so that the long loops run for the lanes
//    that need them;
//  * the hot, small tables live in LDS next to the stacks: the breadth-first top of the triangle-BVH forest, the
//    object-level heaps, MeshObject roots and sphere centres/radii (k_sched prologue);
//  * the other kernel modes share every device function with the default one (frame_device.h, front_device.h) and exist as
//    measured alternatives and bit-for-bit cross-checks, each in a translation unit of its own: kernels_basic.hip (0 one thread
//    per pixel, 1 one launch per bounce over compacted queues, 2 persistent waves without phase scheduling), kernels_pool.hip
//    (4 a path pool in LDS), kernels_serve.hip (5 the triangle-BVH phase as a service of the workgroup).
// This file holds what a product frame runs: k_sched, the AdditionShader blends, the strip packers, and their launchers.
// Arithmetic is the normative float32 of include/urt_math.h, compiled with -ffp-contract=off; results
// are bit-identical to the scalar restatement in oracle/ (tests/test_gpu_parity.py).
#include "experiments.h"    // first: it looks at the -D switches before any default below is defined
#include "front_device.h"     // frame_device.h (Trace, camera rays, work hand-out) + the object-level phase of modes 3 and 5
#include "launch_host.h"
#include <utility>

namespace {

// ---------------------------------------------------------------------------------------------------
// mode 3: persistent waves, lanes SCHEDULED BY PHASE inside the wave.
// Measured on mode 2 (profiles/README.md): after the first bounce only a minority of a wave's lanes needs
// the triangle-BVH loop and the rest idle through it (18 % VALU lane utilisation).  Here every lane carries
// a small state machine
//     DEAD -> FRONT (ground plane + object-level heap walk) -> BLAS (triangle BVH of one MeshObject)
//          -> RESUME (rest of the heap walk, spheres) -> SHADE -> FRONT (next bounce / ray) | DEAD
// and each trip round the wave loop the 64 lanes vote (ballot) on ONE phase to run.  Cheap phases (SHADE from
// `shade_min` lanes, FRONT, refill from `refill_min` dead lanes) run until at least `blas_min` lanes are parked in
// BLAS, then the traversal loop runs with that many lanes; it hands control back when fewer than `blas_exit` lanes are
// still traversing (their stack lives in LDS and the node cursor in registers, so they resume later).
// In the plain forms (FMODE 0, 1) a new ray does not wait in FRONT for a vote (P.front_fuse, the default): every ray is created at the end
// of a trip — a bounce ray or a pixel's next ray by SHADE / SKY, a camera ray by the refill at the top of the next one — and its fresh
// object-level step runs right after the refill, ahead of the vote, for all of them at once.  So with fusing on
//     DEAD -> (refill + fresh step) -> BLAS | SHADE | SKY;   SHADE / SKY -> (fresh step) -> BLAS | SHADE | SKY | DEAD
// and FRONT trips are voted only for RESUME.  A scene of one heap node and no spheres (front_fuse 2, FMODE 0) takes the fresh step as
// straight-line code (front_device.h front_single) and never resumes, so it votes no FRONT trip at all.  Fusing off (option "front_fuse"
// 0) and the listed and masked forms keep the voted FRONT trip for new rays.
// A workgroup is 4 such waves that share nothing but read-only LDS copies made in the prologue: the breadth-first top
// of the BVH forest (a ray entering a mesh walks it on its own, at LDS latency, before it joins the wave-wide loop —
// inside FRONT when TOPF, i.e. for multi-mesh scenes, else at the start of the BLAS phase) and the small object-level
// tables.  Per-pixel arithmetic and the order of its operations are exactly those of modes 0-2 (same device
// functions) — only WHEN and WHERE a lane executes them changes, so pixels are bit-identical.
// ---------------------------------------------------------------------------------------------------
#ifndef URT_SCHED_OCC
#define URT_SCHED_OCC 5
#endif
// MULTI: _numRays > 1 (the running resultAverage and the ray counter are live path state only then).
// One launch traces P.n_frames consecutive frames (frame table T): a lane whose path has ended takes its next pixel from the
// NEXT frame once the current one is handed out, so only the last frame of a launch pays the drain of the long paths.
// FMODE: how FRONT treats MeshObjects — 0: a ray that must enter a triangle BVH goes to the BLAS phase at once (one mesh);
// 1: it first walks the LDS-resident top of that BVH inside FRONT (several meshes); 2: listed form of 1 (front_listed above).
// QN: the traversal loop reads the 32-byte quantized nodes (S.blas_qnodes; never together with COUNT: the counting instantiation walks
// the float nodes, like the oracle).
// Normal cones (trace_device.h cone_skips, csrc/cones.hip): the instantiations that neither count nor read quantized nodes and-in "the ray does
// not see this child's triangles from behind" into both child hits of every node step, in the walk of the LDS top and in the wave-wide loop.
// The cone words ride in the nodes' two spare dwords and are 0 (never skip) while option "blas_cones" is off, so the instantiation — and its
// name — is the same either way; the counting instantiation walks like the oracle, event for event.
// The tile entry table (tile_entry.h) — FMODE 0 with the cone instantiation only: a camera ray that front_single sends into the mesh starts at
// its tile's entries (front_device.h tile_entry_start).  The table's address rides behind the last entry of the frame table (0: the launch
// has none), so that the kernel's arguments — and with them every other instantiation — stay as they are.
template <bool COUNT, int BLOCK, int FMODE, bool MULTI, bool QN = false>
__global__ __launch_bounds__(BLOCK, URT_SCHED_OCC) void k_sched(DevScene S, FrameParams P, const FrameEntry* __restrict__ T, float4* __restrict__ result, DevCounters* ctr,
                                               unsigned int* __restrict__ next) {
  // LDS of the workgroup: [the tile reservation: 16 B][top of the triangle-BVH forest: top_nodes x 64 B, shared by its waves][tables][stacks of wave 0][wave 1]...
  // Apart from the reservation word (frame_device.h wg_fetch_pixels) the waves of a workgroup share only read-only copies and never synchronise after this prologue.
  constexpr bool CONES = !COUNT && !QN;
  extern __shared__ int lds[];
  float4* lds4 = (float4*)lds;
  const float4* top = lds4 + 1;
  if (threadIdx.x == 0) *(unsigned long long*)lds = run_word(blockIdx.x & ((unsigned int)P.n_shards - 1u), 0, 0, 0, false);   // drained, on the workgroup's home shard
  for (int i = threadIdx.x; i < P.top_nodes * 4; i += blockDim.x) lds4[1 + i] = S.blas_cnodes[i];
  int at = 1 + P.top_nodes * 4;                                 // running offset in float4 units
  FrontLds L;
  if (P.lds_mesh) {                                             // object-level mesh heap + MeshObject roots
    for (int i = threadIdx.x; i < 2 * S.n_mesh_tlas; i += blockDim.x) lds4[at + i] = S.mesh_tlas[i];
    L.mesh_tlas = lds4 + at; at += 2 * S.n_mesh_tlas;
    for (int i = threadIdx.x; i < S.n_meshes; i += blockDim.x) ((int32_t*)(lds4 + at))[i] = S.mesh_root[i];
    L.mesh_root = (const int32_t*)(lds4 + at); at += (S.n_meshes + 3) / 4;
    if (P.lds_small) {                                          // triangle records of the single-leaf MeshObjects (quads, planes)
      for (int i = threadIdx.x; i < S.n_meshes; i += blockDim.x) ((int32_t*)(lds4 + at))[i] = S.mesh_small_first[i];
      L.small_first = (const int32_t*)(lds4 + at); at += (S.n_meshes + 3) / 4;
      for (int m = threadIdx.x; m < S.n_meshes; m += blockDim.x) {
        int sf = S.mesh_small_first[m];
        if (sf >= 0) {
          uint32_t code = ~(uint32_t)S.mesh_root[m];
          uint32_t first = code >> 3, cnt = (code & 7u) + 1u;
          for (uint32_t q = 0; q < 3 * cnt; q++) lds4[at + 3 * sf + q] = S.tri_verts[3 * (size_t)first + q];
        }
      }
      L.small_tris = lds4 + at; at += 3 * S.n_small;
    }
  }
  WalkLds W;
  if (FMODE == 3) {                                             // masked FRONT: the walk table instead of the heap (front_masked)
    const float4* wsrc = S.mesh_tlas + 2 * S.n_mesh_tlas;
    for (int i = threadIdx.x; i < P.walk_f4; i += blockDim.x) lds4[at + i] = wsrc[i];
    W.hdr = (const int*)(lds4 + at); W.pos_tab = W.hdr + 16; W.eval = lds4 + at + 20; at += P.walk_f4;
    if (P.lds_small) {                                          // triangle records of the single-leaf MeshObjects
      for (int m = threadIdx.x; m < S.n_meshes; m += blockDim.x) {
        int sf = S.mesh_small_first[m];
        if (sf >= 0) {
          uint32_t code = ~(uint32_t)S.mesh_root[m];
          uint32_t first = code >> 3, cnt = (code & 7u) + 1u;
          for (uint32_t q = 0; q < 3 * cnt; q++) lds4[at + 3 * sf + q] = S.tri_verts[3 * (size_t)first + q];
        }
      }
      L.small_tris = lds4 + at; at += 3 * S.n_small;
    }
  }
  if (P.lds_sphere) {                                           // object-level sphere heap + sphere positions/radii
    for (int i = threadIdx.x; i < 2 * S.n_sphere_tlas; i += blockDim.x) lds4[at + i] = S.sphere_tlas[i];
    L.sphere_tlas = lds4 + at; at += 2 * S.n_sphere_tlas;
    for (int i = threadIdx.x; i < S.n_spheres; i += blockDim.x) lds4[at + i] = S.sphere_pr[i];
    L.sphere_pr = lds4 + at; at += S.n_spheres;
  }
  __syncthreads();
  int* tl = lds + at * 4 + (threadIdx.x >> 6) * ((P.tlas_stack + P.blas_stack) * 64) + (threadIdx.x & 63);
  int* bl = tl + P.tlas_stack * 64;
  LocalCounters lc;
  unsigned int tiles_per_frame;
  const unsigned int ntiles = launch_tiles(P, tiles_per_frame);
  // the waves of a workgroup draw from ONE shard (and, workgroups b, b + 256, ... landing on the same CU, so does the whole CU):
  // neighbours on the chip work on neighbouring tiles (a shard per wave: C2 +6 %, C3 +4 %, C4 +3 %, C5 +3 % time)
  WorkCursor wc; wc.shard = blockIdx.x & ((unsigned int)P.n_shards - 1u);
  bool exhausted = false;
  int st = ST_DEAD;
  // path state
  int xy = 0;                                    // pixel: x | y << 16 (both < 65536)
  int ray_i = 0, kf = 0;                         // kf: bounce index k | frame of the launch << 24
  float seed = 0;
  v3 o = mk3(0, 0, 0), d = mk3(0, 0, 1), energy = mk3(0, 0, 0), res = mk3(0, 0, 0), avg = mk3(0, 0, 0);
  // trace state (one Trace() in flight per lane)
  HitRec best; best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
  int cs = 0;                                    // object-level heap walk (RS:294-326): stack height `check` | never-reset `tests` flag << 8
  bl[0] = kBlasDone;                                  // the sentinel below every traversal stack of this lane (blas_node_eval_ptr): heights start at 1
  int32_t cur = kBlasDone; int sp = 1, best_i = -1;   // triangle-BVH cursor of the current MeshObject
  unsigned int wave_iters = 0, wave_rays = 0;
  bool watchdog = false;
#ifdef URT_STAMPS
  unsigned long long ph_t[4] = {0, 0, 0, 0}, ph_lanes[4] = {0, 0, 0, 0}, ph_trips[4] = {0, 0, 0, 0};   // FRONT, BLAS, SHADE, blas inner trips
  unsigned long long t_begin = wall_clock64(), t_dry = 0;
  unsigned long long c_begin = __builtin_amdgcn_s_memtime();
  unsigned long long dr_trips[4] = {0, 0, 0, 0}, dr_t[3] = {0, 0, 0}, dr_live = 0, dr_lanes3 = 0;   // after the work ran dry
  unsigned long long fs_arr[7] = {0, 0, 0, 0, 0, 0, 0};   // listed FRONT: time in the heap walk / single-leaf tests / BVH-top walks, walks, single-leaf rounds, top walks, fresh lanes walked
  unsigned long long rf_t[3] = {0, 0, 0};                  // refill: time in the work-counter hand-out (the atomic's round trip), in the camera rays, refills
  unsigned long long rf_adds = 0;                          // refill: device-scope atomics on the work counters
  unsigned long long bl_part[3] = {0, 0, 0};               // BLAS loop: lanes that took part in their trip (sum), node trips, lanes at a leaf during node trips (sum)
#endif

  for (;;) {
    if (watchdog) break;
#ifdef URT_STAMPS
    if (exhausted && !t_dry) t_dry = wall_clock64();
#endif
    unsigned long long mD = wballot(st == ST_DEAD);
    int nD = __popcll(mD);
    int nB = 0, nS = 0, nK = 0, nF = 0;
    if (FMODE >= 2) {                // (the plain forms count their lanes below, after the new rays' first step)
      nB = __popcll(wballot(st == ST_BLAS));
      nS = __popcll(wballot(st == ST_SHADE));
      nK = __popcll(wballot(st == ST_SKY));
      nF = __popcll(wballot(st == ST_FRONT || st == ST_RESUME));
    }
    // ---- refill dead lanes: when enough lanes are dead, or when nothing else is left to run.  From the workgroup's reservation in LDS
    // (P.handout > 0, the default: frame_device.h wg_fetch_pixels — a compare-and-swap there, and one work-counter atomic per reservation, by
    // the wave that drains it), or from the frame's work counter with one atomic per refill (P.handout = 0: wave_fetch_pixels).  That atomic
    // takes 2.3 us to return (7.6 % of a wave's time on C3, profiles/r03_logs/r3_stamps_refill.log) and the whole wave waits for it; the other
    // waves of the SIMD cover only part of the wait (C3 +7 % without it).  Two ways of hiding it inside the wave lost: issuing
    // it a trip early cost +23 % (r3_ab_split_refill.log: lanes stay dead a trip longer), reserving several tiles per wave +4 %
    // (r3_ab_refill_chunk.log: more live state in the loop). ----
    if (!exhausted && nD > 0 && (nD >= P.refill_min || (FMODE < 2 ? nD == 64 : nB + nS + nK + nF == 0))) {   // (every lane is in exactly one state)
      int x = 0, y = 0, frame = 0;
#ifdef URT_STAMPS
      unsigned long long t_rf = wall_clock64();
#endif
#ifdef URT_STAMPS
      bool got = P.handout ? wg_fetch_pixels(P, mD, st == ST_DEAD, next, ntiles, (unsigned long long*)lds, exhausted, x, y, tiles_per_frame, &frame, &rf_adds)
                           : wave_fetch_pixels(P, mD, st == ST_DEAD, next, ntiles, wc, exhausted, x, y, tiles_per_frame, &frame);
      if (!P.handout) rf_adds++;
#else
      bool got = P.handout ? wg_fetch_pixels(P, mD, st == ST_DEAD, next, ntiles, (unsigned long long*)lds, exhausted, x, y, tiles_per_frame, &frame)
                           : wave_fetch_pixels(P, mD, st == ST_DEAD, next, ntiles, wc, exhausted, x, y, tiles_per_frame, &frame);
#endif
#ifdef URT_STAMPS
      rf_t[0] += wall_clock64() - t_rf; t_rf = wall_clock64();
#endif
      for_each_frame(got, frame, [&](int f, bool mine) {
        if (mine) {
          st = ST_FRONT;
          ray_i = 0; kf = frame << 24; xy = x | (y << 16);
          avg = mk3(0, 0, 0); res = mk3(0, 0, 0); energy = mk3(1, 1, 1);
          camera_ray_frame(T, f, P, x, y, true, seed, o, d);
        }
      });
#ifdef URT_STAMPS
      rf_t[1] += wall_clock64() - t_rf; rf_t[2]++;
#endif
      if (FMODE >= 2) {
        nF = __popcll(wballot(st == ST_FRONT || st == ST_RESUME));
        nD = __popcll(wballot(st == ST_DEAD));
      }
    }
    bool fresh_pass = false;
    if constexpr (FMODE < 2) {
      // ---- fused FRONT (P.front_fuse): every ray is born in ST_FRONT in the trip that just ended — a bounce ray or a pixel's next ray at the
      // end of the SHADE / SKY body, a camera ray in the refill above — and a voted FRONT trip would run for these same lanes (44.6 per FRONT
      // trip against 44.4 per SHADE trip, profiles/r12_logs/r12_stamps_cones.log).  So their fresh step runs now, without a vote: the FRONT
      // body below, for the new rays alone, and the lanes count toward `blas_min` in the vote that follows it.  Per ray the same device
      // function with the same operands as in a voted trip; dead lanes run nothing. ----
      if (P.front_fuse) { nF = __popcll(wballot(st == ST_FRONT)); fresh_pass = nF > 0; }
      if (!fresh_pass) {
        nB = __popcll(wballot(st == ST_BLAS));
        nS = __popcll(wballot(st == ST_SHADE));
        nK = __popcll(wballot(st == ST_SKY));
        nF = __popcll(wballot(st == ST_FRONT || st == ST_RESUME));
        nD = 64 - (nB + nS + nK + nF);
      }
    }
    bool can_refill = !exhausted && nD >= P.refill_min;
    if (++wave_iters > P.sched_trips) { watchdog = true; break; }   // an exit every wave reaches, whatever the data
    int phase;
    int exit_below = 1;              // traversal runs to completion unless other lanes can make progress meanwhile
    // Surface shading is the longest straight-line code (~750 VALU whatever the lane count, the sky lookup ~270): a thin batch
    // waits while the FRONT phase can still feed it.  P.shade_split: surface hits and misses are separate phases with their
    // own thresholds (fuller lanes per trip; pays when FRONT is cheap, i.e. one mesh); otherwise they count together and
    // run back to back in one trip, so that FRONT — the expensive phase of multi-mesh scenes — gets all of them at once.
    bool sky_too = false;
    if (fresh_pass) phase = ST_FRONT;
    else if (nB >= P.blas_min) { phase = ST_BLAS; if (nS + nK + nF > 0 || can_refill) exit_below = min(P.blas_exit, nB); }   // <= nB: the phase always advances a lane
    else if (P.shade_split) {
      if (nS >= P.shade_min) phase = ST_SHADE;
      else if (nK >= P.sky_min) phase = ST_SKY;
      else if (nF > 0) phase = ST_FRONT;
      else if (nS > 0 && nS >= nK) phase = ST_SHADE;
      else if (nK > 0) phase = ST_SKY;
      else if (nB > 0) phase = ST_BLAS;
      else if (exhausted) break;       // every lane dead and no work left
      else continue;                   // every fetched slot fell outside the region: fetch again
    }
    else if (nS + nK >= P.shade_min) { phase = nS > 0 ? ST_SHADE : ST_SKY; sky_too = true; }
    else if (nF > 0) phase = ST_FRONT;
    else if (nS + nK > 0) { phase = nS > 0 ? ST_SHADE : ST_SKY; sky_too = true; }
    else if (nB > 0) phase = ST_BLAS;
    else if (exhausted) break;       // every lane dead and no work left
    else continue;                   // every fetched slot fell outside the region: fetch again

#ifdef URT_STAMPS
    unsigned long long t_ph = wall_clock64();
    int ph_id = phase == ST_FRONT ? 0 : phase == ST_BLAS ? 1 : 2;
    ph_lanes[ph_id] += (unsigned long long)(phase == ST_FRONT ? nF : phase == ST_BLAS ? nB : phase == ST_SHADE ? nS : nK);
    ph_trips[ph_id]++;
    if (exhausted) { if (!dr_live) dr_live = 64 - nD; dr_trips[ph_id]++; }
#endif
    if (phase == ST_FRONT) {
      // ---------------- FRONT / RESUME: Trace() up to the next triangle-BVH visit (RS:364-383) ----------------
      if (FMODE < 2) wave_rays += (unsigned int)__popcll(wballot(st == ST_FRONT));     // Trace() invocations (RS:454), counted per wave
      if (FMODE >= 2) {
        bool mine = st == ST_FRONT || st == ST_RESUME;
        int r = FMODE == 3 ? front_masked<COUNT, 1, CONES>(S, P, mine, st == ST_FRONT, o, d, best, cs, tl, cur, lc, L, W, top, bl, sp, wave_rays URT_FS_ARG)
                           : front_listed<COUNT, 1, CONES>(S, P, mine, st == ST_FRONT, o, d, best, cs, tl, cur, lc, L, top, bl, sp, wave_rays URT_FS_ARG);
        if (mine && r != 2) {
          if (r == 1) { best_i = -1; st = ST_BLAS; }
          else st = best.t < URT_INF ? ST_SHADE : ST_SKY;
        }
      } else if (st == ST_FRONT || (!fresh_pass && st == ST_RESUME)) {
        sp = 1;
        bool need;
        if (FMODE == 0 && fresh_pass && P.front_fuse == 2) {
          need = front_single<COUNT>(S, o, d, best, cs, cur, lc, L);
          if constexpr (FMODE == 0 && CONES) {
            if (need && (kf & 0xffffff) == 0) {                 // a camera ray: from its tile's entries
              const int4* te = launch_tile_entry_table(T, P.n_frames);
              if (te) need = tile_entry_start(te, P.width, xy, bl, cur, sp);
            }
          }
        } else {
          int check = cs & 0xff; bool seen = (cs >> 8) != 0;
          need = FMODE == 1 ? trace_front<COUNT, true, false, 1, CONES>(S, st == ST_FRONT, o, d, best, check, seen, tl, 64, cur, lc, L, top, P.top_nodes, bl, &sp)
                            : trace_front<COUNT, false, false, 1>(S, st == ST_FRONT, o, d, best, check, seen, tl, 64, cur, lc, L);
          cs = check | (seen ? 256 : 0);
        }
        if (need) { best_i = -1; st = ST_BLAS; }
        else st = best.t < URT_INF ? ST_SHADE : ST_SKY;
      }
    } else if (phase == ST_BLAS) {
      // ---------------- BLAS: triangle BVH of one MeshObject, resumable ----------------
      bool mine = st == ST_BLAS;
      BlasRay R = blas_ray(o, d);
      // A ray that has just entered a MeshObject first walks the LDS-resident top of the forest (nodes [0, top_nodes)) on its
      // own, at LDS latency: the first ~6 of its ~12 node visits then never wait for another lane's cache miss.  Same
      // visits in the same order as the wave-wide loop below would make; far children go on the lane's stack as usual.
      int* spp = bl + (sp - 1) * 64;                         // the top entry of the lane's stack: what a pop returns (height 1 = the sentinel)
      const int rw = CONES ? cone_ray_word(d) : 0;           // the ray's word of the cone test: one register, live across the loop
      if (mine && cur >= 0 && cur < P.top_nodes) {           // (pointer-form stack here too: no address arithmetic per step)
        do {
          if (COUNT) lc.blas_nodes++;
          const float4* n = top + 4 * cur;
          cur = CONES ? blas_node_eval_cone_ptr(n[0], n[1], n[2], n[3], R, best.t, rw, spp) : blas_node_eval_ptr(n[0], n[1], n[2], n[3], R, best.t, spp);
        } while (cur >= 0 && cur < P.top_nodes);
      }
      // The loop works on ONE integer per lane: c = the cursor of the lanes that take part, kBlasDone for every other lane.  Both
      // votes are then single compares whose result IS the ballot (kBlasDone is negative, so c >= 0 <=> an interior node of a
      // participating lane), and the loop control sits in scalar registers (the limits are pinned there).
      int32_t c = mine ? cur : kBlasDone;
      int budget = __builtin_amdgcn_readfirstlane((int)min(P.watchdog_steps, 0x7fffffffu));   // trips left before the watchdog ends this phase (counted down: no kernel argument in the loop)
      const int exit_s = __builtin_amdgcn_readfirstlane(exit_below);
      QRay Q;
      if (QN) Q = make_qray(o, d, S.blas_qnodes[0], S.blas_qnodes[1]);     // the grid frame: two wave-uniform loads per phase entry
      for (;;) {
        int nA = __popcll(wballot(c != kBlasDone));
        if (nA < exit_s) break;
        if (--budget < 0) { watchdog = true; break; }
#ifdef URT_STAMPS
        ph_trips[3]++; ph_lanes[3] += (unsigned long long)nA;
        if (exhausted) { dr_trips[3]++; dr_lanes3 += (unsigned long long)nA; }
#endif
        // majority vote: this trip runs EITHER the interior-node step OR the leaf step, for the lanes that hold that kind
        // of cursor (the others wait one trip) — so a trip costs one of the two bodies, not their sum.
        int nI = __popcll(wballot(c >= 0));
        bool node_trip = 2 * nI >= nA;             // (weighting the vote 1/3 or 2/3: +0.4 % / +2 %; a minority step: +4 ... +7 % — profiles/r03_logs/r3_ab_vote_xload.log, r3_ab_minority.log)
#ifdef URT_STAMPS
        bl_part[0] += (unsigned long long)(node_trip ? nI : nA - nI); bl_part[1] += node_trip ? 1 : 0; bl_part[2] += (unsigned long long)(node_trip ? nA - nI : 0);
#endif
        if (node_trip) {
          if (QN) {
            if (c >= 0) {
              const float4* n = (const float4*)((const char*)(S.blas_qnodes + 2) + ((uint32_t)c << 5));
              float4 u0 = n[0], u1 = n[1];
              c = qnode_eval_ptr(u0, u1, Q, best.t, spp);
            }
          } else if (c >= 0) {
            if (COUNT) lc.blas_nodes++;
            const float4* n = (const float4*)((const char*)S.blas_cnodes + ((uint32_t)c << 6));
            float4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
            c = CONES ? blas_node_eval_cone_ptr(q0, q1, q2, q3, R, best.t, rw, spp) : blas_node_eval_ptr(q0, q1, q2, q3, R, best.t, spp);
          }
        } else if (c < 0 && c != kBlasDone) {
          test_leaf<COUNT>(S, c, o, d, best, best_i, lc);
          c = *spp; spp -= 64;                               // pop (the sentinel ends the traversal)
        }
      }
      if (mine) { cur = c; sp = ((int)(spp - bl) >> 6) + 1; }
      // back to the heap walk (RS:323-325 continues) — or, when nothing of Trace() is left to do (empty object-level stack and
      // no spheres), straight to shading: saves the path one scheduling round trip per bounce
      if (mine && cur == kBlasDone) st = ((FMODE == 3 ? cs : (cs & 0xff)) == 0 && S.n_spheres == 0) ? (best.t < URT_INF ? ST_SHADE : ST_SKY) : ST_RESUME;
    } else {
      // ---------------- SHADE + bookkeeping of CSMain's loops (RS:444-468) ----------------
      bool next_ray = false;
      bool cont = false, shaded = false;
      if (phase == ST_SHADE) {                              // surface hits
        if (st == ST_SHADE) { shaded = true; cont = shade_surface<COUNT>(S, best, o, d, energy, res, seed, (float)(xy & 0xffff), (float)((unsigned)xy >> 16), lc); }
      }
      if (phase == ST_SKY || (sky_too && nK > 0)) {         // misses
        if (st == ST_SKY) { shaded = true; cont = shade_sky<COUNT>(S, d, energy, res, lc); }
      }
      if (shaded) {
        kf++;
        st = ST_FRONT;
        if (!cont || (kf & 0xffffff) >= P.num_bounces) {    // RS:453,457-460
          v3 sum = (MULTI ? avg : mk3(0, 0, 0)) + res;       // RS:464
          if (MULTI) { avg = sum; ray_i++; next_ray = ray_i < P.num_rays; }
          if (!next_ray) {
            float n = (float)P.num_rays;                      // (!MULTI: n = 1 and x / 1 = x — no divisions)
            st_nt(result + (size_t)((unsigned)kf >> 24) * P.frame_stride + (size_t)((unsigned)xy >> 16) * P.width + (xy & 0xffff),
                      MULTI ? make_float4(sum.x / n, sum.y / n, sum.z / n, 1.0f) : make_float4(sum.x, sum.y, sum.z, 1.0f));   // RS:468
            st = ST_DEAD;
          }
        }
      }
      if (MULTI) {                                          // RS:444: next ray of the pixel, _Seed carries over
        for_each_frame(next_ray, (int)((unsigned)kf >> 24), [&](int f, bool mine) {
          if (mine) {
            res = mk3(0, 0, 0); energy = mk3(1, 1, 1); kf &= (int)0xff000000;
            camera_ray_frame(T, f, P, xy & 0xffff, (int)((unsigned)xy >> 16), false, seed, o, d);
          }
        });
      }
    }
#ifdef URT_STAMPS
    ph_t[ph_id] += wall_clock64() - t_ph;
    if (exhausted) dr_t[ph_id] += wall_clock64() - t_ph;
#endif
  }
#ifdef URT_STAMPS
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* sp_ = (unsigned long long*)(next + kWorkShards * 32);
    size_t w = ((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 32;
    for (int q = 0; q < 4; q++) sp_[w + 16 + q] = dr_trips[q];
    for (int q = 0; q < 3; q++) sp_[w + 20 + q] = dr_t[q];
    sp_[w + 23] = dr_live; sp_[w + 24] = dr_lanes3;
    for (int q = 0; q < 4; q++) { sp_[w + q] = ph_t[q]; sp_[w + 4 + q] = ph_lanes[q]; sp_[w + 8 + q] = ph_trips[q]; }
    sp_[w + 12] = t_begin; sp_[w + 13] = wall_clock64(); sp_[w + 14] = t_dry; sp_[w + 15] = __builtin_amdgcn_s_memtime() - c_begin;
    for (int q = 0; q < 7; q++) sp_[w + 25 + q] = fs_arr[q];
    if (FMODE < 2) { sp_[w + 25] = rf_t[0]; sp_[w + 26] = rf_t[1]; sp_[w + 27] = rf_t[2] | (rf_adds << 32); sp_[w + 28] = 0; sp_[w + 29] = bl_part[0]; sp_[w + 30] = bl_part[1]; sp_[w + 31] = bl_part[2]; }     // (single-mesh instantiations: no FRONT split, the refill's instead; slot 27: refills | work-counter atomics << 32)
  }
#endif
  if (watchdog && (threadIdx.x & 63) == 0) report_watchdog(P, ctr);
  lc.rays = (threadIdx.x & 63) == 0 ? wave_rays : 0u;
  flush_counters<COUNT>(lc, ctr);
}

// ---------------------------------------------------------------------------------------------------
// AdditionShader — AS:9,39-41 as driven by RM:817-818.  dst = src*a + dst*(1-a), a = 1/(sample+1);
// the fragment's alpha is a itself.  16 B per lane, grid-stride.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blit_add(const float4* __restrict__ src, float4* __restrict__ dst, size_t n, float sample) {
  float a = 1.0f / (sample + 1.0f);
  float ia = 1.0f - a;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float4 t = src[i], c = dst[i];
    c.x = t.x * a + c.x * ia;
    c.y = t.y * a + c.y * ia;
    c.z = t.z * a + c.z * ia;
    c.w = a * a + c.w * ia;
    dst[i] = c;
  }
}

// n consecutive blends in one pass (frames of a batched launch): per pixel the SAME operations in the same order as n
// k_blit_add launches, with 16 (n + 2) bytes of traffic per pixel instead of 48 n.
// `present` (may be null): the image the host presents the accumulated frame to after every blend (Graphics.Blit(_converged,
// destination), RM:819).  Of the n presents of a fused run only the last is observable (every observer of `present` submits the
// deferred work first, frame_batch.cpp), so the last blended value is stored to both images: the bytes a copy of dst would carry.
struct BlendSamples { float s[kMaxFramesPerLaunch]; };
__global__ __launch_bounds__(256) void k_blit_add_multi(const float4* __restrict__ src, size_t frame_stride, int n, BlendSamples smp,
                                                        float4* __restrict__ dst, float4* __restrict__ present, size_t npix) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    float4 c = dst[i];
    for (int f = 0; f < n; f++) {
      float a = 1.0f / (smp.s[f] + 1.0f);
      float ia = 1.0f - a;
      float4 t = src[(size_t)f * frame_stride + i];
      c.x = t.x * a + c.x * ia;
      c.y = t.y * a + c.y * ia;
      c.z = t.z * a + c.z * ia;
      c.w = a * a + c.w * ia;
    }
    dst[i] = c;
    if (present) present[i] = c;
  }
}

// strips <-> dense buffer (frame-end gather): strip j of this rank = pixel rows (first + j*stride)*8 .. +8
__global__ __launch_bounds__(256) void k_pack_rows(const float4* __restrict__ img, float4* __restrict__ dense, int width, int height,
                                                   int first_group_row, int row_stride, int n_strips, int to_dense) {
  size_t per_strip = (size_t)width * 8;
  size_t n = per_strip * (size_t)n_strips;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int j = (int)(i / per_strip);
    size_t r = i - (size_t)j * per_strip;
    int row = (first_group_row + j * row_stride) * 8 + (int)(r / (size_t)width);
    int col = (int)(r % (size_t)width);
    if (row < height) {
      size_t at = (size_t)row * width + col;
      if (to_dense) dense[i] = img[at]; else const_cast<float4*>(img)[at] = dense[i];
    } else if (to_dense) {
      dense[i] = make_float4(0, 0, 0, 0);
    }
  }
}

// The same strips with THREE channels per pixel (12 B): the frame-end gather of a running mean need not move its alpha channel — after
// sample n it is the same value in every pixel, a function of the sample sequence alone (AS:40: the fragment's alpha is a itself and is
// blended like the colours) — so the root writes `alpha` itself when it de-interleaves.  A quarter of the gather's bytes less.
__global__ __launch_bounds__(256) void k_pack_rows_rgb(const float4* __restrict__ img, float* __restrict__ dense, int width, int height,
                                                       int first_group_row, int row_stride, int n_strips, int to_dense, float alpha) {
  size_t per_strip = (size_t)width * 8;
  size_t n = per_strip * (size_t)n_strips;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int j = (int)(i / per_strip);
    size_t r = i - (size_t)j * per_strip;
    int row = (first_group_row + j * row_stride) * 8 + (int)(r / (size_t)width);
    int col = (int)(r % (size_t)width);
    float* d = dense + 3 * i;
    if (row < height) {
      size_t at = (size_t)row * width + col;
      if (to_dense) { float4 v = img[at]; d[0] = v.x; d[1] = v.y; d[2] = v.z; }
      else const_cast<float4*>(img)[at] = make_float4(d[0], d[1], d[2], alpha);
    } else if (to_dense) {
      d[0] = 0; d[1] = 0; d[2] = 0;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// host-side launchers (declared in kernels.h)
// ---------------------------------------------------------------------------------------------------
namespace urtd {

// The dynamic LDS of one workgroup of modes 3 and 5: the prologue of k_sched (and of kernels_serve.hip k_serve) restated as a size, table by
// table in the same order and in its float4 units — a table added there is added here
size_t sched_lds_bytes(const DevScene& S, const FrameParams& P) {
  size_t f4 = (size_t)P.top_nodes * 4;
  if (P.lds_mesh) f4 += 2 * (size_t)S.n_mesh_tlas + ((size_t)S.n_meshes + 3) / 4;
  if (P.walk_f4 > 0) f4 += (size_t)P.walk_f4 + (P.lds_small ? 3 * (size_t)S.n_small : 0);       // masked FRONT: the walk table replaces the heap (lds_mesh = 0)
  else if (P.lds_small) f4 += ((size_t)S.n_meshes + 3) / 4 + 3 * (size_t)S.n_small;
  if (P.lds_sphere) f4 += 2 * (size_t)S.n_sphere_tlas + (size_t)S.n_spheres;
  if (P.serve) f4 += 2 * (size_t)P.block_threads + 1;          // mode 5: the workgroup's mailbox (k_serve)
  else f4 += 1;                                                // mode 3: the workgroup's tile reservation (frame_device.h wg_fetch_pixels)
  return f4 * 16 + (size_t)(P.tlas_stack + P.blas_stack) * 64 * (size_t)(P.block_threads / 64) * sizeof(int);
}

// The k_sched instantiation for the runtime values: entry i of a table over (COUNT, MULTI, QN, FMODE 0-3, BLOCK 64 / 256), bit by bit.
// QN never comes with COUNT (the counting instantiation walks the float nodes, like the oracle): those entries are not instantiated.
using SchedKernel = void (*)(DevScene, FrameParams, const FrameEntry*, float4*, DevCounters*, unsigned int*);
template <int I>
static constexpr SchedKernel sched_entry() {
  constexpr bool COUNT = (I & 1) != 0, MULTI = (I & 2) != 0, QN = (I & 4) != 0;
  if constexpr (COUNT && QN) return nullptr;
  else return k_sched<COUNT, (I & 32) ? 256 : 64, (I >> 3) & 3, MULTI, QN>;
}
template <int... I>
static SchedKernel sched_kernel(bool count, int block, int fmode, bool multi, bool qn, std::integer_sequence<int, I...>) {
  static const SchedKernel table[] = {sched_entry<I>()...};
  return table[(count ? 1 : 0) | (multi ? 2 : 0) | (qn ? 4 : 0) | (fmode << 3) | (block == 256 ? 32 : 0)];
}

hipError_t launch_sched(const DevScene& S, const FrameParams& P, const FrameEntry* T, float4* result, DevCounters* ctr,
                        unsigned int* next, int n_blocks, int front_mode, bool count, hipStream_t st, TraceLaunchRecord* rec) {
  if (n_blocks <= 0) return hipSuccess;
  if (P.block_threads != 64 && P.block_threads != 256) return hipErrorInvalidValue;   // independent waves; a workgroup shares the LDS top-of-tree copy
  if (!batched_args_ok(S, P, front_mode)) return hipErrorInvalidValue;
  if (front_mode == 3 && (P.walk_f4 < 20 || P.lds_mesh || P.top_nodes <= 0 || S.n_mesh_tlas > 31)) return hipErrorInvalidValue;
  if (front_mode != 3 && P.walk_f4 != 0) return hipErrorInvalidValue;
  hipError_t e = reset_work_counters(next, st);
  if (e != hipSuccess) return e;
  const int block = P.block_threads;
  const int fmode = front_mode < 1 || front_mode > 3 || (front_mode == 1 && P.top_nodes <= 0) ? 0 : front_mode;
  const bool multi = P.num_rays > 1, qn = !count && S.blas_qnodes;
  return launch_traced(named(rec, "k_sched<%s, %d, %d, %s, %s>", tf(count), block, fmode, tf(multi), tf(qn)),
                       sched_kernel(count, block, fmode, multi, qn, std::make_integer_sequence<int, 64>()),
                       n_blocks, block, sched_lds_bytes(S, P), st, S, P, T, result, ctr, next);
}

hipError_t launch_blit_add(const float4* src, float4* dst, size_t n_pixels, float sample, hipStream_t st) {
  if (n_pixels == 0) return hipSuccess;
  size_t nb = (n_pixels + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_blit_add, dim3((unsigned)nb), dim3(256), 0, st, src, dst, n_pixels, sample);
  return hipGetLastError();
}

hipError_t launch_blit_add_multi(const float4* src, size_t frame_stride, int n, const float* samples, float4* dst, float4* present,
                                 size_t n_pixels, hipStream_t st) {
  if (n_pixels == 0 || n <= 0) return hipSuccess;
  if (n > kMaxFramesPerLaunch) return hipErrorInvalidValue;
  BlendSamples smp{};
  for (int f = 0; f < n; f++) smp.s[f] = samples[f];
  size_t nb = (n_pixels + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_blit_add_multi, dim3((unsigned)nb), dim3(256), 0, st, src, frame_stride, n, smp, dst, present, n_pixels);
  return hipGetLastError();
}

hipError_t launch_pack_rows(float4* img, float4* dense, int width, int height, int first_group_row, int row_stride,
                            int n_strips, bool to_dense, hipStream_t st) {
  size_t n = (size_t)width * 8 * (size_t)n_strips;
  if (n == 0) return hipSuccess;
  size_t nb = (n + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)nb), dim3(256), 0, st, (const float4*)img, dense, width, height,
                     first_group_row, row_stride, n_strips, to_dense ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_pack_rows_rgb(float4* img, float* dense, int width, int height, int first_group_row, int row_stride,
                                int n_strips, bool to_dense, float alpha, hipStream_t st) {
  size_t n = (size_t)width * 8 * (size_t)n_strips;
  if (n == 0) return hipSuccess;
  size_t nb = (n + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(k_pack_rows_rgb, dim3((unsigned)nb), dim3(256), 0, st, (const float4*)img, dense, width, height,
                     first_group_row, row_stride, n_strips, to_dense ? 1 : 0, alpha);
  return hipGetLastError();
}

}  // namespace urtd
