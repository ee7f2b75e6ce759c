// frame_batch.cpp — dispatch of the trace kernels: deferred frames and their Result slab, launch configuration, the trace launch
// itself and the deferred blends / presents / strip packs behind it (context_impl.h: "frame batching", "Overlapped launches").
#include "experiments.h"
#include "context_impl.h"

#include "reproject.h"
#include "tile_entry.h"

namespace urtd {

// Scheduler trips a wave of a persistent kernel may make before it gives up (kernels.hip).  A frame needs 1e3-1e5; the cap
// grows with what the launch carries: frames x (rays x bounces / 8).
static unsigned int sched_trip_cap(urt_context* ctx, const FrameParams& P, int n_frames) {
  if (ctx->opt.watchdog_cap > 0) return (unsigned int)ctx->opt.watchdog_cap;
  uint64_t per = std::max<uint64_t>(1, (uint64_t)std::max(1, P.num_rays) * (uint64_t)std::max(1, P.num_bounces) / 8u);
  uint64_t cap = (1ull << 24) * (uint64_t)std::max(1, n_frames) * per;
  return (unsigned int)std::min<uint64_t>(cap, 0xfffffff0ull);
}

static int ensure_queues(urt_context* ctx, size_t n_paths, size_t n_counts) {   // (the wait for the main stream at growth is new; the launch that follows touches it anyway)
  for (int k = 0; k < 8; k++) {
    if (int rc = reserve(ctx, ctx->q_store[k / 4][k % 4], n_paths, "path queue allocation", touch(ctx))) return rc;
    ctx->q.s[k / 4][k % 4] = ctx->q_store[k / 4][k % 4].get();
  }
  if (int rc = reserve(ctx, ctx->q_counts, n_counts, "path queue allocation", touch(ctx))) return rc;
  ctx->q.counts = ctx->q_counts.get();
  return URT_OK;
}

int resolve_timing(urt_context* ctx) {
  for (auto& pr : ctx->timing) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, pr.first.get(), pr.second.get()) == hipSuccess) ctx->trace_ms += ms;
    ctx->event_pool.push_back(std::move(pr.first));
    ctx->event_pool.push_back(std::move(pr.second));
  }
  ctx->timing.clear();
  return URT_OK;
}

static int take_event(urt_context* ctx, Event* out) {
  if (!ctx->event_pool.empty()) { *out = std::move(ctx->event_pool.back()); ctx->event_pool.pop_back(); return URT_OK; }
  URT_HIP(ctx, out->create(hipEventDefault));
  return URT_OK;
}

// ---- Result renaming: the slab of frame slots ---------------------------------------------------------------------------
bool in_slab(urt_context* ctx, const Texture& t) {
  return ctx->slab && t.dev >= ctx->slab.get() && t.dev < ctx->slab.get() + ctx->slab_stride * (size_t)ctx->slab_frames;
}

// Give a texture its own storage back (its current contents are copied out of the slab slot they live in).
int detach_from_slab(urt_context* ctx, Texture& t) {
  if (!in_slab(ctx, t)) return URT_OK;
  URT_HIP(ctx, hipMemcpyAsync(t.own, t.dev, (size_t)t.w * t.h * sizeof(float4), hipMemcpyDeviceToDevice, touch(ctx)));
  t.dev = t.own;
  return URT_OK;
}

// Slab of `frames` zero-filled slots for texture `h` (all work queued so far stays ordered before its first use: same stream).
static int ensure_slab(urt_context* ctx, urt_handle h, Texture& t, int frames) {
  size_t stride = (size_t)t.w * (size_t)t.h;
  if (ctx->slab && ctx->slab_tex == h && ctx->slab_stride == stride && ctx->slab_frames >= frames) return URT_OK;
  // two slots of this size did not fit last time: not tried per frame — but again after a release in this context (free_scene,
  // urt_texture_release clear the mark) and every 256th dispatch (another context on the card may have given memory back);
  // urt_debug_launch_info reports the degradation (slab_frames_max, slab_out_of_memory)
  if (!ctx->slab && ctx->slab_oom_stride == stride && (ctx->dispatches & 255u) != 0) return URT_OK;
  if (ctx->slab_tex) {                                   // somebody's current contents may live in the old slab
    auto it = ctx->textures.find(ctx->slab_tex);
    if (it != ctx->textures.end()) { int rc = detach_from_slab(ctx, it->second); if (rc) return rc; }
    ctx->slab_tex = 0;
  }
  if (!ctx->slab || ctx->slab_stride * (size_t)ctx->slab_frames < stride * (size_t)frames) {
    if (ctx->slab) {
      URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));   // queued kernels may still use the old slab
      ctx->slab.reset(); ctx->slab_frames = 0; ctx->slab_stride = 0;
    }
    // out of memory (several contexts on one card, a huge image): halve the batch until the slots fit; one frame = no slab at
    // all (the caller then renders unbatched, straight into the texture)
    hipError_t e = hipErrorOutOfMemory;
    while (frames >= 2) {
      e = ctx->slab.alloc(stride * (size_t)frames);
      if (e != hipErrorOutOfMemory) break;
      frames /= 2;
    }
    if (e == hipErrorOutOfMemory) { ctx->slab_frames = 0; ctx->slab_stride = 0; ctx->slab_frames_max = 1; ctx->slab_oom_stride = stride; return URT_OK; }
    URT_HIP(ctx, e);
    ctx->slab_frames = frames;
    ctx->slab_frames_max = frames;
  } else {
    ctx->slab_frames = (int)(ctx->slab_stride * (size_t)ctx->slab_frames / stride);    // same bytes, re-cut for this image size
  }
  ctx->slab_stride = stride;
  if (ctx->slab_frames < 2) return URT_OK;               // (re-cut for a larger image: no room for two slots -> unbatched)
  URT_HIP(ctx, hipMemsetAsync(ctx->slab.get(), 0, stride * (size_t)ctx->slab_frames * sizeof(float4), touch(ctx)));   // a new RenderTexture is zero-filled
  ctx->slab_tex = h;
  return URT_OK;
}

// Persistent kernels: a work-counter shard hands out RUNS of consecutive 8x8 tiles (and the waves of a workgroup share a shard),
// so neighbours on the chip work on neighbouring tiles.  Run length when "xcd_run" is 0 (auto): the largest power of two <= 8 that
// leaves every shard >= 256 runs per launch.  Measured with the frames of a launch interleaved (profiles/r02_logs/r2_run_by_launch.log, C3):
// one frame per launch 0.62 ms at 1 vs 0.82 at 64 (few runs per shard: the shards run dry unevenly); 16 frames 0.24 vs 0.33;
// 64 frames 0.221 at 4-8 vs 0.224 at 64.  (Before the interleaving, runs of 64 were the gain: r2_xcd_run.log.)
static int auto_run_length(const FrameParams& P, int n_frames) {
  long runs = (long)P.tiles_x * P.n_strips * std::max(1, n_frames) / ((long)std::max(1, P.n_shards) * 256L);
  int g = 1;
  while (g < 8 && 2L * g <= runs) g *= 2;
  return g;
}

// Mode 3, option "handout": tiles per reservation of a workgroup (FrameParams::handout), 0 = per-wave atomics.  The largest divisor of the
// run length that is at most 16 (1024 slots: the reservation word counts slots in 11 bits), so that a reservation never leaves its run —
// the auto run lengths 1 .. 8 are handed out whole.  Mode 5 keeps the dword for pool_inloop; frames of 2^24 tiles and more keep the counters.
static void set_handout(urt_context* ctx, FrameParams& P) {
  if (P.serve) return;
  int c = 0;
  if (ctx->opt.handout != 0 && (uint64_t)P.tiles_x * (uint64_t)P.n_strips + (uint64_t)P.xcd_run < (1u << 24)) {
    c = std::min(P.xcd_run, 16);
    while (P.xcd_run % c) c--;
  }
  P.handout = c;
}

// One attempt at `groups` workgroups per CU; *degraded = an LDS feature the scene qualifies for had to be given up (or the stacks alone do not fit)
static int configure_sched_at(urt_context* ctx, const DevScene& S, FrameParams& P, bool top_in_front, size_t groups, bool* degraded) {
  // independent waves; the waves of a workgroup share one LDS copy of the top of the triangle-BVH forest, which shrinks
  // until the workgroups fit the 160 KiB of a CU next to their traversal stacks
  int t = std::min(std::min(ctx->opt.top_nodes >= 0 ? ctx->opt.top_nodes : 64, (int)kTopOrderNodes), ctx->scene.n_blas_nodes);
  // small object-level tables (<= 256 entries) also live in LDS: their walk is a chain of dependent fetches
  P.lds_mesh = ctx->opt.lds_tlas && S.n_mesh_tlas > 0 && S.n_mesh_tlas <= 256 && S.n_meshes <= 256;
  P.lds_small = P.lds_mesh && S.n_small > 0;
  P.lds_sphere = ctx->opt.lds_tlas && S.n_sphere_tlas > 0 && S.n_sphere_tlas <= 256 && S.n_spheres <= 256;
  const bool wanted_tables = P.lds_mesh || P.lds_sphere;
  P.top_nodes = t;
  const size_t budget = 156 * 1024;                          // (a little of the 160 KiB goes to allocation granules)
  while (P.top_nodes > 0 && sched_lds_bytes(S, P) * groups > budget) P.top_nodes /= 2;
  if (ctx->opt.top_nodes < 0 && P.top_nodes == 64) {
    // auto: what is left of the workgroup's share of the LDS holds more of the forest's top, 16 nodes (1 KiB) at a time — C3 / C3D: 96 nodes,
    // -0.6 % per frame in 64-frame launches (profiles/r04_logs/r4_sweep_top_nodes.log); every node there is a fetch at LDS latency
    const int most = std::min((int)kTopOrderNodes, ctx->scene.n_blas_nodes);
    while (P.top_nodes + 16 <= most) {
      P.top_nodes += 16;
      if (sched_lds_bytes(S, P) * groups > budget) { P.top_nodes -= 16; break; }
    }
  }
  if (sched_lds_bytes(S, P) * groups > budget) { P.lds_mesh = 0; P.lds_sphere = 0; P.lds_small = 0; }
  *degraded = (t > 0 && P.top_nodes == 0) || (wanted_tables && !(P.lds_mesh || P.lds_sphere)) || sched_lds_bytes(S, P) * groups > budget;
  // listed FRONT (front_device.h front_listed): scenes of a few MeshObjects whose heap is in LDS; the list of objects a ray has to test
  // (<= 12 ids of 5 bits) lives in the first two entries of the lane's object-level stack, so it costs no LDS
  bool listed = top_in_front && P.top_nodes > 0 && P.lds_mesh && S.n_meshes <= 12 && ctx->opt.front_list != 0;
  // masked FRONT (front_device.h front_masked): mesh heaps of <= 31 nodes are walked with mask arithmetic instead of a stack; the walk
  // table takes the heap's place in LDS.  "front_list" 2 forces the listed form (A/B), -1 / 1 prefer the masked one.
  bool masked = top_in_front && t > 0 && ctx->opt.lds_tlas && ctx->scene.walk_f4 > 0 && !P.serve && ctx->opt.front_list != 0 && ctx->opt.front_list != 2;
  if (masked) {
    // The masked walk keeps no object-level stack for the mesh heap: the lane's `tl` column only serves the sphere heap's walk.  The
    // entries that frees (C4, C5: 4 of 6, i.e. 4 KiB per workgroup) go to the LDS copy of the top of the forest, which is sized again for this layout.
    FrameParams Q = P;
    Q.lds_mesh = 0; Q.walk_f4 = ctx->scene.walk_f4; Q.lds_small = S.n_small > 0;
    Q.tlas_stack = std::max(2, heap_levels(S.n_sphere_tlas) + 1);
    Q.top_nodes = t;
    if (ctx->opt.top_nodes < 0) {
      // measured (profiles/r03_logs/r3_sweep_top_masked.log): C4 (3 big MeshObjects) 2.97 / 2.99 / 3.01 / 3.06 ms at a top of 4 / 8 / 16 / 64 nodes,
      // C5 (12) 1.57 / 1.52 / 1.50 / 1.495 / 1.50 at 4 / 8 / 16 / 32 / 64: the roots and about one more level
      int big = 0;
      for (int32_t r : ctx->scene.h_mesh_root) big += r >= 0 && r != kEmptyMeshRoot;
      int want = 4;
      while (want < 2 * big && want < 64) want *= 2;
      Q.top_nodes = std::min(t, want);
    }
    while (Q.top_nodes > 0 && sched_lds_bytes(S, Q) * groups > budget) Q.top_nodes /= 2;
    if (Q.top_nodes > 0 && sched_lds_bytes(S, Q) * groups <= budget) { P = Q; *degraded = false; return 3; }
    *degraded = true;
  }
  return listed ? 2 : (top_in_front && P.top_nodes > 0) ? 1 : 0;
}

// kernel_mode 3: what lives in the workgroup's LDS next to the stacks (fills P.top_nodes, P.lds_*, P.block_threads, P.list_base,
// P.tlas_stack), how many workgroups per CU the launch counts on (ctx->sched_groups) and how FRONT treats MeshObjects (returns the
// front mode of kernels.h launch_sched).  5 waves per SIMD (what 96 VGPRs allow) = 5 workgroups of 4 waves per CU is the target; a scene
// whose traversal stacks are too deep for that (a GPU-built Morton tree of 100 k triangles is 30 levels: 34 KiB of stacks per workgroup)
// keeps its LDS features — the masked object-level phase, the tables, the top of the forest — at 4 or 3 workgroups per CU instead
// of losing them at a nominal 5 that the hardware would not make resident anyway (GPU-built trees: C4 6.71 -> 3.61 ms, C3 0.284 -> 0.264, C3D 0.502 -> 0.443; profiles/r03_logs/r3_lbvh_groups.log).
static int configure_sched(urt_context* ctx, const DevScene& S, FrameParams& P, bool top_in_front) {
  {
    const int t = std::min(std::min(ctx->opt.top_nodes >= 0 ? ctx->opt.top_nodes : 64, (int)kTopOrderNodes), ctx->scene.n_blas_nodes);
    const bool lds_mesh = ctx->opt.lds_tlas && S.n_mesh_tlas > 0 && S.n_mesh_tlas <= 256 && S.n_meshes <= 256;
    const bool lds_sphere = ctx->opt.lds_tlas && S.n_sphere_tlas > 0 && S.n_sphere_tlas <= 256 && S.n_spheres <= 256;
    const bool shared = t > 0 || lds_mesh || lds_sphere;
    P.block_threads = ctx->opt.sched_block > 0 ? ctx->opt.sched_block : (shared ? 256 : 64);   // nothing to share: single waves
    if (P.serve) P.block_threads = 256;                        // kernel_mode 5: the waves of a workgroup share the traversal service
  }
  const int wpc_default = P.serve ? 16 : 20;                 // what the kernel's registers allow (k_serve: 128 VGPRs, k_sched: 96)
  const size_t per = (size_t)(P.block_threads / 64);
  const size_t groups = std::max<size_t>(1, (size_t)(ctx->opt.waves_per_cu > 0 ? ctx->opt.waves_per_cu : wpc_default) / per);   // workgroups per CU that should fit
  ctx->sched_groups = 0;
  const FrameParams P0 = P;
  bool degraded = false;
  int mode = configure_sched_at(ctx, S, P, top_in_front, groups, &degraded);
  if (degraded && ctx->opt.waves_per_cu <= 0 && per == 4) {
    for (size_t g = groups - 1; g >= 3 && g + 2 >= groups; g--) {
      FrameParams Q = P0; bool d2 = false;
      int m2 = configure_sched_at(ctx, S, Q, top_in_front, g, &d2);
      if (!d2) { P = Q; mode = m2; ctx->sched_groups = (int)g; break; }
    }
  }
  return mode;
}

// What urt_debug_launch_info reports: the record a launcher of kernels.h filled, and the launch's configuration
static void record_launch(urt_context* ctx, const TraceLaunchRecord& R, int kernel_mode, int front_mode, const FrameParams& P, bool count, int waves_per_cu) {
  urt_launch_info& I = ctx->last_launch;
  std::memset(&I, 0, sizeof I);
  std::snprintf(I.kernel, sizeof I.kernel, "%s", R.kernel);
  I.kernel_mode = kernel_mode; I.front_mode = front_mode; I.count_stats = count ? 1 : 0;
  I.n_blocks = R.n_blocks; I.block_threads = R.block_threads; I.lds_bytes = R.lds_bytes;
  I.n_frames = P.n_frames; I.frame_group = P.frame_group; I.xcd_run = P.xcd_run; I.tile_order = P.tile_order;
  I.top_nodes = P.top_nodes; I.waves_per_cu = waves_per_cu;
  I.tlas_stack = P.tlas_stack; I.blas_stack = P.blas_stack;
  I.lds_tables = (P.lds_mesh ? 1 : 0) | (P.lds_sphere ? 2 : 0) | (P.lds_small ? 4 : 0) | (P.walk_f4 > 0 ? 8 : 0);
  I.slab_frames = ctx->slab_frames; I.slab_frames_max = ctx->slab_frames_max; I.slab_out_of_memory = ctx->slab_oom_stride != 0 ? 1 : 0;
  I.experiment = URT_ABI_SIGN < 0 ? 1 : 0;
  I.handout = kernel_mode == 3 ? P.handout : 0;
}

// One trace launch on stream `st`: `launch(TraceLaunchRecord*)` enqueues it through a launcher of kernels.h, between two timing events
// when "time_dispatch" is on; then the launch is counted and recorded (record_launch)
template <typename Launch>
static int timed_launch(urt_context* ctx, hipStream_t st, int kernel_mode, int front_mode, const FrameParams& P, bool count, int waves_per_cu, Launch launch) {
  Event e0, e1;
  if (ctx->opt.time_dispatch) {
    int rc = take_event(ctx, &e0); if (rc) return rc;
    rc = take_event(ctx, &e1); if (rc) return rc;
    URT_HIP(ctx, hipEventRecord(e0.get(), st));
  }
  TraceLaunchRecord rec{};
  hipError_t le = launch(&rec);
  if (ctx->opt.time_dispatch) {
    (void)hipEventRecord(e1.get(), st);
    ctx->timing.emplace_back(std::move(e0), std::move(e1));
  }
  ctx->launches++;
  if (le != hipSuccess) return fail(ctx, URT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(le));
  record_launch(ctx, rec, kernel_mode, front_mode, P, count, waves_per_cu);
  return URT_OK;
}

// ---- The tile entry table (csrc/tile_entry.h) -----------------------------------------------------------------------------------------------
// What a dispatch can tell of a launch's right to the table before its frames are known: the plain single-mesh form of kernel_mode 3, in the
// instantiation that applies the cones' rule (not counting, no quantized nodes).  do_dispatch gives such a launch the stack entries
// tile_entry_start stores to.
static bool tile_entry_form(const urt_context* ctx, const DevScene& S, bool count, bool serve, bool top_in_front) {
  return ctx->opt.tile_entry != 0 && ctx->opt.front_fuse != 0 && !serve && !top_in_front && !count && !S.blas_qnodes && S.blas_cnodes && S.mesh_tlas &&
         S.mesh_root && S.n_mesh_tlas == 1 && S.n_meshes > 0 && S.n_spheres == 0 && ctx->scene.n_blas_nodes > 0;
}

// The table for this launch, or null when the launch runs without one: every frame must have frame 0's camera, bit for bit, and pixel
// offsets in [0, 1] (the sample rectangle tile_entry.h derives its frustum from).  Cached by camera, image size and node contents; a miss
// builds it on `st`, behind the launches on the other streams that still read the old one.
static int tile_entry_for_launch(urt_context* ctx, const DevScene& S, const FrameParams& P, const FrameTable& T, int front_mode, bool count,
                                 hipStream_t st, const int32_t** out) {
  *out = nullptr;
  if (front_mode != 0 || P.front_fuse != 2 || P.blas_stack < kTileEntryK || !tile_entry_form(ctx, S, count, P.serve != 0, false)) return URT_OK;
  const FrameUniforms& u0 = T.f[0].u;
  for (int f = 0; f < P.n_frames; f++) {
    const FrameUniforms& u = T.f[f].u;
    if (std::memcmp(u.c2w, u0.c2w, sizeof u.c2w) != 0 || std::memcmp(u.invp, u0.invp, sizeof u.invp) != 0) return URT_OK;
    if (!(u.pixel_off_x >= 0.0f && u.pixel_off_x <= 1.0f && u.pixel_off_y >= 0.0f && u.pixel_off_y <= 1.0f)) return URT_OK;
  }
  urt_context::TileEntryKey key{};
  std::memcpy(key.c2w, u0.c2w, sizeof key.c2w); std::memcpy(key.invp, u0.invp, sizeof key.invp);
  key.width = P.width; key.height = P.height; key.scene_epoch = ctx->scene_epoch; key.nodes_epoch = ctx->nodes_epoch; key.nodes = S.blas_cnodes;
  const int si = ctx->trace_q[0] && st == ctx->trace_q[0].get() ? 1 : ctx->trace_q[1] && st == ctx->trace_q[1].get() ? 2 : 0;
  if (!ctx->te_ready) {
    URT_HIP(ctx, ctx->te_ready.create(hipEventDisableTiming));
    for (Event& ev : ctx->te_used) URT_HIP(ctx, ev.create(hipEventDisableTiming));
  }
  // auto: a table is built for a camera that has demonstrably stood still — a launch of two frames or more, or the key of the previous launch —
  // so that a host whose camera moves with every submitted frame does not pay a pre-pass per frame (0.57 ms at 1080p on C3)
  const bool still = P.n_frames >= 2 || (ctx->te_seen && std::memcmp(&key, &ctx->te_seen_key, sizeof key) == 0);
  ctx->te_seen_key = key; ctx->te_seen = true;
  if (!ctx->te_valid || std::memcmp(&key, &ctx->te_key, sizeof key) != 0) {
    if (ctx->opt.tile_entry < 0 && !still) return URT_OK;
    ctx->te_valid = false;
    const size_t words = (size_t)((P.width + 7) / 8) * (size_t)((P.height + 7) / 8) * kTileEntryK;
    for (int k = 0; k < 3; k++) {                            // the readers of the old table, wherever they run
      if (!ctx->te_used_set[k]) continue;
      if (words > ctx->te_table.cap()) URT_HIP(ctx, hipEventSynchronize(ctx->te_used[k].get()));
      else if (k != si) URT_HIP(ctx, hipStreamWaitEvent(st, ctx->te_used[k].get(), 0));
      ctx->te_used_set[k] = false;
    }
    if (int rc = reserve(ctx, ctx->te_table, words, "tile entry table", nullptr)) return rc;
    URT_HIP(ctx, launch_tile_entry(S, ctx->scene.n_blas_nodes, key.c2w, key.invp, P.width, P.height, ctx->te_table.get(), st));
    URT_HIP(ctx, hipEventRecord(ctx->te_ready.get(), st));
    ctx->te_key = key; ctx->te_valid = true; ctx->te_stream = st; ctx->te_builds++;
  } else if (st != ctx->te_stream) {
    URT_HIP(ctx, hipStreamWaitEvent(st, ctx->te_ready.get(), 0));
  }
  *out = ctx->te_table.get();
  return URT_OK;
}

// Launch the phase-scheduled trace kernel for P.n_frames frames (uniforms T) into result + f * P.frame_stride.
static constexpr int kAutoFrames = 64;     // frames per launch when "frames_per_launch" is 0 (auto) on the library's own stream

static int launch_sched_frames(urt_context* ctx, const DevScene& S, const FrameParams& P, const FrameTable& T, float4* result,
                        int front_mode, bool count, hipStream_t st = nullptr, unsigned int* next = nullptr) {
  if (!st) { st = touch(ctx); next = ctx->d_next.get(); }       // the main stream; flush_pending may pass one of its trace streams and that stream's work counters
  // the launch's frame table -> device memory, in stream order (pinned staging slot: the copy does not wait for the stream)
  if (!ctx->h_tables) {
    URT_HIP(ctx, ctx->h_tables.alloc((size_t)urt_context::kTableSlotEntries * urt_context::kTableSlots));
    URT_HIP(ctx, ctx->d_tables.alloc((size_t)urt_context::kTableSlotEntries * urt_context::kTableSlots));
    for (Event& ev : ctx->table_ev) URT_HIP(ctx, ev.create(hipEventDisableTiming));
  }
  const unsigned int slot = ctx->table_next++ % (unsigned int)urt_context::kTableSlots;
  if (ctx->table_next > (unsigned int)urt_context::kTableSlots) URT_HIP(ctx, hipEventSynchronize(ctx->table_ev[slot].get()));   // (four launches ago: long done)
  FrameEntry* h_slot = ctx->h_tables.get() + (size_t)slot * urt_context::kTableSlotEntries;
  FrameEntry* d_table = ctx->d_tables.get() + (size_t)slot * urt_context::kTableSlotEntries;
  const int32_t* te = nullptr;                               // the launch's tile entry table: its address rides behind the last entry (kernels.h launch_sched)
  if (int rc = tile_entry_for_launch(ctx, S, P, T, front_mode, count, st, &te)) return rc;
  const uint64_t te_addr = (uint64_t)(uintptr_t)te;
  std::memcpy(h_slot, T.f, sizeof(FrameEntry) * (size_t)P.n_frames);
  std::memcpy(h_slot + P.n_frames, &te_addr, sizeof te_addr);
  URT_HIP(ctx, hipMemcpyAsync(d_table, h_slot, sizeof(FrameEntry) * (size_t)P.n_frames + sizeof te_addr, hipMemcpyHostToDevice, st));
  URT_HIP(ctx, hipEventRecord(ctx->table_ev[slot].get(), st));
  int waves_per_block = P.block_threads / 64;
  long want = ((long)P.tiles_x * P.n_strips * P.n_frames + waves_per_block - 1) / waves_per_block;
  // resident waves per CU: every slot the registers allow (k_sched: 96 VGPRs -> 5 waves/SIMD = 20 per CU).  While the
  // frame's work counter was one address, fewer and fatter waves were faster at 1080p (12 per CU); since it is sharded
  // (frame_device.h wave_fetch_pixels) the full 20 win at every frame size measured (profiles/README.md).
  int wpc = ctx->opt.waves_per_cu;
  if (wpc <= 0) wpc = P.serve ? 16 : 20;
  if (ctx->sched_groups > 0) wpc = ctx->sched_groups * waves_per_block;       // deep stacks: fewer workgroups per CU, LDS features kept (configure_sched)
  long resident = (long)ctx->n_cus * wpc / waves_per_block;
  int nb = (int)std::max(1L, std::min(want, resident));
  if (P.serve) {                                             // mailbox of the posted rays: 32 B per thread of the grid
    if (int rc = reserve(ctx, ctx->d_mail, (size_t)nb * (size_t)P.block_threads * 2, "mailbox allocation", touch(ctx))) return rc;
  }
  int rc = timed_launch(ctx, st, P.serve ? 5 : 3, front_mode, P, count, wpc, [&](TraceLaunchRecord* rec) {
    return P.serve ? launch_serve(S, P, d_table, result, ctx->d_counters.get(), next, ctx->d_mail.get(), nb, front_mode, count, st, rec)
                   : launch_sched(S, P, d_table, result, ctx->d_counters.get(), next, nb, front_mode, count, st, rec);
  });
  if (te) {                                                    // a later rebuild of the table waits for this launch
    const int si = ctx->trace_q[0] && st == ctx->trace_q[0].get() ? 1 : ctx->trace_q[1] && st == ctx->trace_q[1].get() ? 2 : 0;
    URT_HIP(ctx, hipEventRecord(ctx->te_used[si].get(), st));
    ctx->te_used_set[si] = true;
  }
  if (rc == URT_OK) { ctx->last_launch.tile_entry = te ? 1 : 0; ctx->last_launch.tile_entry_k = te ? kTileEntryK : 0; }
  // the cone test runs in the instantiations of k_sched that neither count nor read quantized nodes (kernels.hip), on the words of this scene
  if (rc == URT_OK) ctx->last_launch.cones = !P.serve && !count && !S.blas_qnodes && S.blas_cnodes && ctx->scene.cones_in_use ? 1 : 0;
  return rc;
}

// The run of deferred blends that starts at ops[i], which flush_pending makes ONE pass (the same per-pixel operations in the same order):
// blends of the same kind into the same dst (history blends: also the same count and max_history; an additive blend has 0, 0) of
// consecutive frames, up to kMaxFramesPerLaunch, each possibly followed by the present of dst (RM:818-819) — a copy that reads dst and
// writes the run's one target, none of dst, count and the batch's Result `result_tex`.  Only the last present is observable: every call
// that could observe the target submits this work first (as-if rule, include/urt.h); the run ends at that present, so the image
// presented is the one it was presented with.  `samples` receives the _Sample of the additive blends.
struct BlendRun { int frames; urt_handle present; size_t end; };   // present: 0 = none; end: the index after the run
static BlendRun blend_run(const std::vector<PostOp>& ops, size_t i, urt_handle result_tex, float* samples) {
  const PostOp& op = ops[i];
  size_t j = i, j_present = i;
  int cnt = 0, cnt_present = 0;
  urt_handle present = 0;
  while (j < ops.size() && cnt <= kMaxFramesPerLaunch) {
    const PostOp& q = ops[j];
    if (q.kind == op.kind && q.dst == op.dst && q.count == op.count && q.max_history == op.max_history && q.frame == op.frame + cnt &&
        cnt < kMaxFramesPerLaunch) { samples[cnt++] = q.sample; j++; }
    else if (q.kind == OpKind::Copy && q.src == op.dst && q.dst != op.dst && q.dst != op.count && q.dst != result_tex && (present == 0 || q.dst == present)) {
      present = q.dst; j++; j_present = j; cnt_present = cnt;
    } else break;
  }
  if (present) return BlendRun{cnt_present, present, j_present};
  return BlendRun{cnt, 0, j};
}

// Submit the deferred frames: ONE trace launch, then the deferred operations in program order, each run of blends (blend_run) in one pass.
int flush_pending(urt_context* ctx) {
  urt_context::Pending& B = ctx->pend;
  if (B.n == 0) return URT_OK;
  int n = B.n;
  B.n = 0;                                               // whatever happens below, the batch is gone
  std::vector<PostOp> ops;
  ops.swap(B.ops);
  URT_HIP(ctx, hipSetDevice(ctx->device));
  FrameParams P = B.P;
  P.n_frames = n;
  P.sched_trips = sched_trip_cap(ctx, P, n);
  P.frame_group = std::max(1, std::min(P.frame_group, n));
  if (ctx->opt.xcd_run <= 0) P.xcd_run = auto_run_length(P, n);
  set_handout(ctx, P);
  P.frame_stride = (unsigned int)ctx->slab_stride;
  // Small launches (a host that presents every frame) overlap: see urt_context "Overlapped launches".  Launch L goes to trace stream
  // L mod 2 and takes slots [base, base + n) round-robin; it waits for
  //   - pre_ev of launch L-1: everything the main stream held when L-1 was submitted — the blends / presents of L-2 and older (the last
  //     readers of any slot L may reuse), scene uploads, texture writes — but NOT launch L-1 itself nor its blends, whose slots are others;
  //   - or, when anything but the frame loop's own work went to the main stream since (main_touched: SetData, a scene preparation, a
  //     blit outside a batch, a gather, ...) or the slots would collide, for the main stream as it is now — which has waited for L-1.
  // The main stream waits for the launch before its deferred blits, so "the main stream is idle" still means "everything is done".
  int base = 0;
  bool reading = false;                                  // a pipelined readback in flight: the host paces itself on FINISHED frames, and two launches sharing
  for (const auto& r : ctx->rslot) reading = reading || r.busy;   // the chip finish later than one after the other (measured: +6 % C3, +21 % C2 with two tickets in flight)
  const bool eligible = (ctx->opt.overlap_launches == 2 || (ctx->opt.overlap_launches == 1 && !reading)) && ctx->stream == ctx->own_stream.get() && !P.serve && !ctx->opt.time_dispatch &&
                        n <= urt_context::kOverlapFrames && ctx->slab_frames >= 2 * urt_context::kOverlapFrames && ctx->d_next2;
  if (eligible) {
    base = ctx->slab_cursor + n <= ctx->slab_frames ? ctx->slab_cursor : 0;
    if (!ctx->trace_q[0]) {
      for (int k = 0; k < 2; k++) {
        URT_HIP(ctx, ctx->trace_q[k].create(hipStreamNonBlocking));
        URT_HIP(ctx, ctx->trace_done[k].create(hipEventDisableTiming));
        URT_HIP(ctx, ctx->pre_ev[k].create(hipEventDisableTiming));
      }
      URT_HIP(ctx, ctx->dep_ev.create(hipEventDisableTiming));
    }
    const unsigned int k = ctx->trace_parity++ & 1u;
    const bool disjoint = base >= ctx->prev_base + ctx->prev_n || base + n <= ctx->prev_base;
    // A launch's dependency covers every image it READS, not only its Result slots: besides the scene that is the sky.  A texture launch
    // L-1 traced into, or one its deferred blends / copies / presents write (after pre_ev), may have been bound as _SkyboxTexture since.
    const float4* const prev_slots = ctx->slab.get() + (size_t)ctx->prev_base * ctx->slab_stride;
    bool sky_written = B.S.sky >= prev_slots && B.S.sky < prev_slots + (size_t)ctx->prev_n * ctx->slab_stride;
    for (const float4* w : ctx->prev_writes) sky_written = sky_written || w == B.S.sky;
    const bool wide = ctx->main_touched || !disjoint || sky_written;
    if (wide) {
      URT_HIP(ctx, hipEventRecord(ctx->dep_ev.get(), ctx->stream));
      URT_HIP(ctx, hipStreamWaitEvent(ctx->trace_q[k].get(), ctx->dep_ev.get(), 0));
    } else {
      URT_HIP(ctx, hipStreamWaitEvent(ctx->trace_q[k].get(), ctx->pre_ev[k ^ 1u].get(), 0));
      ctx->overlapped_launches++;
    }
    const bool narrow = !wide;
    int rc = launch_sched_frames(ctx, B.S, P, B.T, ctx->slab.get() + (size_t)base * ctx->slab_stride, B.front_mode, B.count, ctx->trace_q[k].get(), (k ? ctx->d_next2 : ctx->d_next).get());
    if (rc) { ctx->main_touched = true; return rc; }
    ctx->last_launch.trace_stream = 1 + (int)k; ctx->last_launch.slab_base = base; ctx->last_launch.overlapped = narrow ? 1 : 0;
    URT_HIP(ctx, hipEventRecord(ctx->trace_done[k].get(), ctx->trace_q[k].get()));
    URT_HIP(ctx, hipEventRecord(ctx->pre_ev[k].get(), ctx->stream));
    URT_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->trace_done[k].get(), 0));
    ctx->main_touched = false;
  } else {
    int rc = launch_sched_frames(ctx, B.S, P, B.T, ctx->slab.get(), B.front_mode, B.count);     // on the main stream (marks it touched)
    if (rc) return rc;
  }
  ctx->prev_base = base; ctx->prev_n = n; ctx->slab_cursor = base + n;
  ctx->prev_writes.clear();                              // (filled below, as the deferred operations are enqueued)
  if (base) {                                            // the Result texture names the LAST frame's slot (do_dispatch named it assuming slot 0)
    Texture* rt = find_texture(ctx, B.tex);
    if (rt && in_slab(ctx, *rt)) rt->dev = ctx->slab.get() + (size_t)(base + n - 1) * ctx->slab_stride;
  }
  const float4* const slots = ctx->slab.get() + (size_t)base * ctx->slab_stride;
  size_t i = 0;
  while (i < ops.size()) {
    const PostOp& op = ops[i];
    if (op.kind == OpKind::BlendAdd || op.kind == OpKind::BlendHistory) {
      const bool history = op.kind == OpKind::BlendHistory;
      Texture* d = find_texture(ctx, op.dst);
      Texture* c = history ? find_texture(ctx, op.count) : nullptr;
      if (!d || (history && !c))
        return fail(ctx, URT_ERR_INVALID_HANDLE, history ? "deferred blit_add_history: texture was released" : "deferred Blit: destination texture was released");
      float samples[kMaxFramesPerLaunch];
      const BlendRun run = blend_run(ops, i, B.tex, samples);
      float4* pdev = nullptr;
      if (run.present) {
        Texture* pt = find_texture(ctx, run.present);
        if (!pt) return fail(ctx, URT_ERR_INVALID_HANDLE, "deferred Blit: destination texture was released");
        pdev = pt->dev;
        ctx->prev_writes.push_back(pdev);
      }
      ctx->prev_writes.push_back(d->dev);
      if (history) ctx->prev_writes.push_back(c->dev);
      const float4* src = slots + (size_t)op.frame * ctx->slab_stride;
      const size_t npix = (size_t)d->w * d->h;
      const bool single = run.frames == 1 && !pdev;
      hipError_t e;
      if (history) e = single ? launch_blit_add_history(src, d->dev, c->dev, npix, op.max_history, ctx->stream)
                              : launch_blit_add_history_multi(src, ctx->slab_stride, run.frames, d->dev, c->dev, pdev, npix, op.max_history, ctx->stream);
      else e = single ? launch_blit_add(src, d->dev, npix, samples[0], ctx->stream)
                      : launch_blit_add_multi(src, ctx->slab_stride, run.frames, samples, d->dev, pdev, npix, ctx->stream);
      if (e != hipSuccess) return fail(ctx, URT_ERR_HIP, std::string(history ? "deferred blit_add_history: " : "deferred Blit: ") + hipGetErrorString(e));
      i = run.end;
    } else if (op.kind == OpKind::Copy) {
      Texture* t = find_texture(ctx, op.src);
      Texture* d = find_texture(ctx, op.dst);
      if (!t || !d) return fail(ctx, URT_ERR_INVALID_HANDLE, "deferred Blit: texture was released");
      const float4* img = op.src == B.tex ? slots + (size_t)op.frame * ctx->slab_stride : t->dev;
      ctx->prev_writes.push_back(d->dev);
      URT_HIP(ctx, hipMemcpyAsync(d->dev, img, (size_t)t->w * t->h * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
      i++;
    } else {
      Texture* t = find_texture(ctx, op.src);
      if (!t) return fail(ctx, URT_ERR_INVALID_HANDLE, "deferred pack_rows: texture was released");
      const float4* img = op.src == B.tex ? slots + (size_t)op.frame * ctx->slab_stride : t->dev;
      int n_strips = strip_count((t->h + 7) / 8, op.first_row, op.row_stride);
      hipError_t e = op.rgb ? launch_pack_rows_rgb(const_cast<float4*>(img), (float*)op.dense, t->w, t->h, op.first_row, op.row_stride, n_strips, true, 0.0f, ctx->stream)
                            : launch_pack_rows(const_cast<float4*>(img), (float4*)op.dense, t->w, t->h, op.first_row, op.row_stride, n_strips, true, ctx->stream);
      if (e != hipSuccess) return fail(ctx, URT_ERR_HIP, std::string("deferred pack_rows: ") + hipGetErrorString(e));
      i++;
    }
  }
  return URT_OK;
}

// frames one launch may hold for this dispatch
static int batch_limit(urt_context* ctx, const FrameParams& P) {
  int lim = ctx->opt.frames_per_launch;
  if (lim == 0) {
    if (ctx->stream != ctx->own_stream.get()) return 1;        // a caller that shares its stream expects the work ON the stream when dispatch returns
    // kAutoFrames frames per launch, within 8 GiB of Result slots: 2160p still gains from long launches (profiles/r02_logs/r2_fpl4k.log),
    // and 32 x 133 MB is nothing on a 288 GB part
    uint64_t frame_bytes = (uint64_t)P.width * (uint64_t)P.height * sizeof(float4);
    lim = (int)std::min<uint64_t>(kAutoFrames, std::max<uint64_t>(1, (8ull << 30) / std::max<uint64_t>(1, frame_bytes)));
  }
  // the work counter hands out 32-bit pixel slots: frames x tiles x 64 must stay below 2^32
  uint64_t slots = std::max<uint64_t>(1, ((uint64_t)P.tiles_x * (uint64_t)P.n_strips + (uint64_t)std::max(64, ctx->opt.xcd_run)) * 64u);   // (a frame's last run is padded when frames are interleaved)
  lim = (int)std::min<uint64_t>((uint64_t)lim, std::max<uint64_t>(1, 0xfffffffeull / slots / 2));
  return std::max(1, std::min(lim, (int)kMaxFramesPerLaunch));
}

// The sky the kernels sample: the texture bound as _SkyboxTexture, or one black texel (an unbound SRV reads zeros).
int bind_sky(urt_context* ctx, DevScene& S) {
  Texture* sky = find_texture(ctx, ctx->t_sky);
  if (sky) { S.sky = sky->dev; S.sky_w = sky->w; S.sky_h = sky->h; }
  else {     // an unbound SRV reads zeros
    if (!ctx->zero_sky) {
      URT_HIP(ctx, ctx->zero_sky.alloc(1));
      URT_HIP(ctx, hipMemsetAsync(ctx->zero_sky.get(), 0, sizeof(float4), touch(ctx)));
    }
    S.sky = ctx->zero_sky.get(); S.sky_w = 1; S.sky_h = 1;
  }
  return URT_OK;
}

int do_dispatch(urt_context* ctx, int kernel, int gx, int gy, int gz, int first_row, int row_stride) {
  if (kernel != 0) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "kernel index must be 0 (CSMain)");
  if (gx < 0 || gy < 0 || gz < 0 || first_row < 0 || row_stride < 1)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "negative thread-group count or bad strip arguments");
  urt_handle res_h = ctx->t_result;
  Texture* res = find_texture(ctx, res_h);
  if (!res) return fail(ctx, URT_ERR_UNBOUND, "Dispatch: no texture bound to \"Result\" (RM:803)");
  if (res->w > 65535 || res->h > 65535) return fail(ctx, URT_ERR_INVALID_ARGUMENT, "Result larger than 65535 pixels per side");
  URT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = current_scene(ctx)) return rc;
  ctx->dispatches++;
  if (gx == 0 || gy == 0 || gz == 0) return URT_OK;

  DevScene S = ctx->scene.ds;
  { int rc = bind_sky(ctx, S); if (rc) return rc; }

  FrameParams P{};
  std::memcpy(P.c2w, ctx->c2w, sizeof P.c2w);
  std::memcpy(P.invp, ctx->invp, sizeof P.invp);
  P.pixel_off_x = ctx->pixel_off[0]; P.pixel_off_y = ctx->pixel_off[1];
  P.seed = ctx->seed;
  P.num_bounces = ctx->num_bounces; P.num_rays = ctx->num_rays;
  P.width = res->w; P.height = res->h;
  long rw = std::min<long>((long)gx * 8, res->w), rh = std::min<long>((long)gy * 8, res->h);
  P.region_w = (int)rw; P.region_h = (int)rh;
  P.tiles_x = (P.region_w + 7) / 8;
  P.first_group_row = first_row; P.row_stride = row_stride;
  P.n_strips = strip_count((P.region_h + 7) / 8, first_row, row_stride);      // rows of the dispatched region
  P.tlas_stack = lane_stack_size(ctx).tlas; P.blas_stack = lane_stack_size(ctx).blas; P.watchdog_steps = ctx->scene.watchdog_steps;
  P.block_threads = ctx->opt.block_threads; P.xcd_run = ctx->opt.xcd_run; P.tile_order = ctx->opt.tile_order >= 0 ? ctx->opt.tile_order : (S.n_meshes == 0 ? 1 : 0); P.refill_min = ctx->opt.refill_min;
  // lanes parked at a triangle BVH before the traversal phase runs: 16 with one mesh (C3 -2 %, C3D -6 % against 28), 24 when rays walk
  // several (C4, C5 -1 %) — re-measured after the work distribution became local (profiles/r02_logs/r2_blas_min.log)
  P.blas_min = ctx->opt.blas_min > 0 ? ctx->opt.blas_min : (S.n_meshes > 1 ? 24 : 16);
  // the traversal phase yields when fewer lanes than this are still traversing: measured best 14-18 with one mesh, 8-11 when rays
  // walk several triangle BVHs per Trace() (a yielding lane then continues its object-level walk sooner)
  P.blas_exit = ctx->opt.blas_exit > 0 ? ctx->opt.blas_exit : (S.n_meshes > 1 ? 9 : 14); P.shade_min = ctx->opt.shade_min; P.sky_min = ctx->opt.sky_min;
  P.n_frames = 1; P.frame_stride = 0;
  P.sched_trips = sched_trip_cap(ctx, P, 1); P.trip_flag = ctx->d_trip_flag;
  if (P.n_strips == 0 || P.tiles_x == 0) return URT_OK;
  P.n_shards = ctx->opt.work_shards; P.frame_group = ctx->opt.frame_group;
  if (ctx->opt.xcd_run <= 0) P.xcd_run = ctx->opt.kernel_mode >= 2 ? auto_run_length(P, 1) : 1;   // (batched launches: again at submission, with the launch's frame count)
  if ((uint64_t)P.tiles_x * (uint64_t)P.n_strips * 64u >= 0xffffffffull)
    return fail(ctx, URT_ERR_INVALID_ARGUMENT, "Dispatch: too many pixel slots in one dispatch");

  // region pixels this dispatch writes (threads outside Result write nothing, RS:468)
  {
    uint64_t px = 0;
    for (int j = 0; j < P.n_strips; j++) {
      int y0 = (first_row + j * row_stride) * 8;
      px += (uint64_t)std::max(0, std::min(P.region_h - y0, 8)) * (uint64_t)P.region_w;
    }
    ctx->pixels_dispatched += px;
  }
  bool degenerate = P.num_bounces <= 0 || P.num_rays <= 0;      // loops that never run: the megakernel handles them literally
  int mode = degenerate ? 0 : ctx->opt.kernel_mode;
  if ((mode == 3 || mode == 5) && P.num_bounces >= (1 << 24)) mode = 2;        // k_sched / k_serve keep the bounce index in 24 bits
  bool count = ctx->opt.count_stats != 0;
  const int region[4] = {P.region_w, P.region_h, first_row, row_stride};
  const bool full_cover = P.region_w == res->w && P.region_h == res->h && first_row == 0 && row_stride == 1;

  if (mode == 3 || mode == 5) {
    bool top_in_front = ctx->opt.top_front < 0 ? S.n_meshes > 1 : ctx->opt.top_front != 0;
    P.serve = mode == 5 && ctx->scene.n_blas_nodes > 0;            // no triangle BVH, nothing to serve: mode 3's kernel
    P.pool_inloop = ctx->opt.serve_refill;
    if (tile_entry_form(ctx, S, count, P.serve != 0, top_in_front)) P.blas_stack = std::max(P.blas_stack, (int)kTileEntryK);   // front_device.h tile_entry_start stores kTileEntryK - 1 entries
    int front_mode = configure_sched(ctx, S, P, top_in_front);
    P.shade_split = ctx->opt.shade_split != 0;
    set_handout(ctx, P);                                          // (batched launches: again at submission, with the launch's run length)
    // plain FRONT: new rays take their first object-level step in the trip that created them; as straight-line code when the mesh heap is one node and there are no spheres
    P.front_fuse = ctx->opt.front_fuse == 0 ? 0 : (S.n_mesh_tlas == 1 && S.n_meshes > 0 && S.n_spheres == 0 ? 2 : 1);
    const FrameUniforms fu = bound_camera(ctx);                   // the uniforms P's head holds
    // May this dispatch be renamed to a fresh slab slot?  Its unwritten pixels must read as before: none (full cover), or
    // still the zeros of creation (only dispatches of this same region ever wrote the image).
    bool same_region = res->n_regions == 1 && std::memcmp(res->rg, region, sizeof region) == 0;
    bool renamable = !res->external && !res->ptr_exposed && (full_cover || (!res->other_writes && (res->n_regions == 0 || same_region)));
    int limit = renamable ? batch_limit(ctx, P) : 1;
    urt_context::Pending& B = ctx->pend;
    if (B.n > 0) {
      const FrameParams& Q = B.P;
      bool same = B.tex == res_h && B.scene_epoch == ctx->scene_epoch && B.S.sky == S.sky && B.S.sky_w == S.sky_w && B.S.sky_h == S.sky_h &&
                  B.count == count && B.front_mode == front_mode && Q.serve == P.serve && Q.num_bounces == P.num_bounces && Q.num_rays == P.num_rays &&
                  Q.width == P.width && Q.height == P.height && Q.region_w == P.region_w && Q.region_h == P.region_h &&
                  Q.first_group_row == P.first_group_row && Q.row_stride == P.row_stride && B.n < B.limit && limit > 1;
      if (!same) { int rc = flush_pending(ctx); if (rc) return rc; }
    }
    if (limit > 1 && B.n == 0) {                          // a new batch: its Result slots (fewer, or none, when memory is short)
      int rc = ensure_slab(ctx, res_h, *res, limit); if (rc) return rc;
      if (!ctx->slab || ctx->slab_tex != res_h || ctx->slab_frames < 2) limit = 1;
    }
    // the flush and the new slab may have given the sky's texture other storage (it was the previous batch's Result, detached just now)
    if (B.n == 0) { int rc = bind_sky(ctx, S); if (rc) return rc; }
    if (limit <= 1) {                                     // not batched: trace this frame now, straight into the texture
      FrameTable T{};
      T.f[0] = frame_entry(fu);
      P.frame_group = 1;
      int rc = launch_sched_frames(ctx, S, P, T, res->dev, front_mode, count);
      if (rc) return rc;
    } else {
      if (B.n == 0) {
        B.limit = std::min(limit, ctx->slab_frames);
        B.tex = res_h; B.scene_epoch = ctx->scene_epoch; B.S = S; B.P = P; B.front_mode = front_mode; B.count = count;
      }
      B.T.f[B.n] = frame_entry(fu);
      res->dev = ctx->slab.get() + (size_t)B.n * ctx->slab_stride;   // Result now names this frame's slot
      B.n++;
    }
  } else {
    int rc = flush_pending(ctx); if (rc) return rc;
    int nb = 0, k = 0;
    if (mode == 1) {
      size_t n_paths = (size_t)P.tiles_x * 64 * (size_t)P.n_strips;
      rc = ensure_queues(ctx, n_paths, (size_t)P.num_rays * (size_t)(P.num_bounces + 1));
      if (rc) return rc;
    } else if (mode == 2) {
      int waves_per_block = P.block_threads / 64;
      long want = ((long)P.tiles_x * P.n_strips + waves_per_block - 1) / waves_per_block;
      int wpc = ctx->opt.waves_per_cu;
      if (wpc <= 0) wpc = 20;
      long resident = (long)ctx->n_cus * wpc / waves_per_block;
      nb = (int)std::max(1L, std::min(want, resident));
    } else if (mode == 4) {
      // one wave per workgroup; residency is bounded by the LDS one wave's path pool takes (kernels_pool.hip k_pool)
      P.block_threads = 64;
      P.refill_min = ctx->opt.pool_refill; P.blas_min = ctx->opt.pool_blas_min; P.blas_exit = ctx->opt.pool_blas_exit;
      P.pool_inloop = ctx->opt.pool_inloop; P.pool_other_min = ctx->opt.pool_other_min;
      k = ctx->opt.pool_k;
      size_t lds = pool_lds_bytes(P, k);
      while (k > 1 && lds > 160 * 1024) { k--; lds = pool_lds_bytes(P, k); }
      if (lds > 160 * 1024) return fail(ctx, URT_ERR_OUT_OF_MEMORY, "kernel_mode 4: the scene's traversal stacks do not fit the LDS of one CU; use kernel_mode 3");
      int fit = (int)std::max<size_t>(1, (160 * 1024) / lds);
      int wpc = ctx->opt.waves_per_cu > 0 ? ctx->opt.waves_per_cu : fit;
      long want = ((long)P.tiles_x * P.n_strips * 64 + 64L * k - 1) / (64L * k);
      nb = (int)std::max(1L, std::min(want, (long)ctx->n_cus * wpc));
    }
    const hipStream_t st = touch(ctx);
    rc = timed_launch(ctx, st, mode, 0, P, count, ctx->opt.waves_per_cu, [&](TraceLaunchRecord* rec) {
      switch (mode) {
        case 1: return launch_wavefront(S, P, ctx->q, res->dev, ctx->d_counters.get(), count, st, rec);
        case 2: return launch_persist(S, P, res->dev, ctx->d_counters.get(), ctx->d_next.get(), nb, count, st, rec);
        case 4: return launch_pool(S, P, res->dev, ctx->d_counters.get(), ctx->d_next.get(), nb, k, count, st, rec);
        default: return launch_mega(S, P, res->dev, ctx->d_counters.get(), count, st, rec);
      }
    });
    if (rc) return rc;
  }
  // remember what has written the image (see Texture)
  if (res->n_regions == 0) { res->n_regions = 1; std::memcpy(res->rg, region, sizeof region); }
  else if (std::memcmp(res->rg, region, sizeof region) != 0) res->n_regions = 2;
  return URT_OK;
}

}  // namespace urtd
