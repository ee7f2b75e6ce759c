// context_impl.h — the context behind the C ABI of include/urt.h, as the translation units that implement it share it:
//   context.cpp      the Unity stand-ins: context lifetime, stream, buffers and their mirrors, textures, readback, uniforms, blits, strip packing, options, counters, debug accessors
//   scene_prep.cpp   bound buffers -> device scene (full and in-place preparation)
//   frame_batch.cpp  deferred frames, the Result slab, trace launches (do_dispatch, flush_pending)
//   image_ops.cpp    ray queries, radiance queries, feature buffers, denoiser, reprojection, upsampling, auto-exposure and tone mapping, depth of field, motion blur, bloom, resampling
//   geometry_ops.cpp skinning, buffer bounds, the object-level BVH on the device, normals plans, morph plans; the buffer-argument checks (BufArg)
//   owned.h          the holders every GPU resource below lives in (DeviceBuf, PinnedBuf, Event, Stream) and `reserve`, the grow-only policy
// Private: nothing else includes it.  What crosses the files lives in namespace urtd and stays hidden (-fvisibility=hidden).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/urt.h"
#include "../../include/urt_math.h"
#include "blas_builder.h"
#include "kernels.h"
#include "owned.h"
#include "urt_device.h"

namespace urtd {

struct Buffer {
  int count = 0, stride = 0;
  std::vector<uint8_t> host;   // SetData copy (RM:250): the caller keeps ownership of its list
  bool has_data = false;
  // elements that differ from what the prepared scene was made from: the union over every SetData / ranged SetData since the last
  // preparation (empty while dirty_last < dirty_first); every preparation clears it
  int dirty_first = 0, dirty_last = -1;
  void mark_dirty(int first, int last) {
    if (dirty_last < dirty_first) { dirty_first = first; dirty_last = last; }
    else { dirty_first = std::min(dirty_first, first); dirty_last = std::max(dirty_last, last); }
  }
  // Optional device mirror (count * stride bytes), made at the first device-side use and initialised from `host`
  // (context.cpp buffer_mirror).  Once it exists it is CURRENT everywhere: a host SetData pushes what it changed on the stream.  Device-side
  // writers (urt_buffer_set_data_device, urt_skin_vertices) leave `host` behind: inside the stale element range (empty while
  // stale_last < stale_first; kept as ONE range like the dirty one, so it may cover elements that are equal on both sides) the mirror is
  // newer, and whatever reads `host` downloads the range first (buffer_sync_host).
  DeviceBuf<char> mirror;
  int stale_first = 0, stale_last = -1;
  uint64_t downloads = 0;        // synchronising device-to-host copies of this buffer since its creation (urt_debug_buffer_state)
  bool stale() const { return stale_last >= stale_first; }
  void mark_stale(int first, int last) {
    if (!stale()) { stale_first = first; stale_last = last; }
    else { stale_first = std::min(stale_first, first); stale_last = std::max(stale_last, last); }
  }
};

struct Texture {
  int w = 0, h = 0;
  float4* dev = nullptr;        // where the CURRENT contents live: `own`, or a frame slot of the context's slab (a Result
                                // texture is renamed to a fresh slot by every batched dispatch)
  float4* own = nullptr;        // the allocation made at creation (or the caller's memory when external)
  DeviceBuf<float4> storage;    // owns `own`; empty when external
  bool external = false;
  bool ptr_exposed = false;     // urt_texture_get_info handed out the device pointer: never renamed again
  // What has written the image since its zero-filled creation.  A dispatch that covers only part of the image may be renamed
  // to a (zero-filled) slab slot only while the pixels outside its region are still the zeros of creation, i.e. while
  // nothing but dispatches of that SAME region has written the image.
  bool other_writes = false;    // SetPixels / Blit destination / unpack_rows
  int n_regions = 0;            // 0 none yet, 1 = every dispatch so far had region `rg`, 2 = mixed
  int rg[4] = {0, 0, 0, 0};     // region_w, region_h, first_group_row, row_stride
};

// urt_normals_plan_create: a normals plan (csrc/normals_plan.h) as the device holds it.  The plan keeps its own validated triangles and
// only the HANDLE of the vertices buffer, looked up at every use.
struct DevNormalsPlan {
  urt_handle vertices = 0;
  int n_vertices = 0;            // the count of the vertices buffer at creation: every index of `tris` lies below it
  urt_NormalsPlanInfo info{};    // what urt_normals_plan_info reports
  DeviceBuf<int32_t> tris, entries, ranges;
};

// urt_morph_plan_create: a morph plan (csrc/morph_plan.h) as the device holds it, entries in plan order: the targets apart from the
// deltas, so that a lane reads an entry's 24 bytes of deltas only when its weight is live (csrc/morph.hip).  It names no buffer.
struct DevMorphPlan {
  urt_MorphPlanInfo info{};              // what urt_morph_plan_info reports
  DeviceBuf<int32_t> ranges, targets;    // {start, length} per served vertex; one target per entry
  DeviceBuf<float> deltas;               // dp[3], dn[3] per entry
};

enum BindSlot { B_MESHOBJECTS, B_VERTICES, B_INDICES, B_NORMALS, B_SPHERES, B_MESHBVH, B_SPHEREBVH, B_COUNT };

}  // namespace urtd

struct urt_context {
  urtd::Stream own_stream;                  // first: destroyed last, after everything that was used on it
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::unordered_map<urt_handle, urtd::Buffer> buffers;
  std::unordered_map<urt_handle, urtd::Texture> textures;
  std::unordered_map<urt_handle, urtd::DevNormalsPlan> normals_plans;
  std::unordered_map<urt_handle, urtd::DevMorphPlan> morph_plans;
  urt_handle next_id = 1;

  urt_handle bound[urtd::B_COUNT] = {0, 0, 0, 0, 0, 0, 0};
  urt_handle t_sky = 0, t_result = 0;
  float c2w[16] = {0}, invp[16] = {0};
  bool c2w_set = false, invp_set = false;  // SetMatrix has given the camera matrices (urt_render_aov needs both)
  float pixel_off[2] = {0, 0};
  float seed = 0;
  int num_bounces = 0, num_rays = 0;     // shader uniforms default to 0 until SetInt (RM:780-781)

  // ---- options (urt_set_option; the table of names and ranges is in context.cpp) ------------------------------------------
  struct Options {
    int refit = 1;                          // 0 = always prepare from scratch
    int refit_vertices = 1;                 // 0 = changed _Vertices / _Normals prepare from scratch (matrix moves are still refitted)
    int refit_rebuild_pct = 0;              // a deformed MeshObject whose tree cost exceeds pct / 100 x its baseline forces a full preparation (0 = never, else > 100)
    int prepare_device = 0;                 // 1 = a full preparation takes _Vertices / _Indices / _Normals from their device mirrors (no download, no host pass over them)
                                            // and always builds on the GPU: the builder asked for when blas_builder >= 1, else 3 (scene_prep.cpp prepare_scene)
    int qnodes = 0;                         // 32-byte quantized nodes in the traversal loop: 0 = off (default: measured -1.3 % on C3 / C3D, +1.3 % on C4 / C5 — the loop waits on the latency of ONE dependent fetch per step, not on its width), 1 = on, -1 = on unless a MeshObject is only a few grid cells wide
    int count_stats = 0, time_dispatch = 0, kernel_mode = 3;
    int block_threads = 64, xcd_run = 0 /* auto */, work_shards = 64, frame_group = 64, refill_min = 16, waves_per_cu = 0 /* auto */, blas_min = 0 /* auto */, blas_exit = 0 /* auto */;
    int pool_k = 2, pool_refill = 32, pool_blas_min = 48, pool_blas_exit = 8, pool_inloop = 16, pool_other_min = 24;   // kernel_mode 4
    int sched_block = 0;                    // kernel_mode 3: threads per workgroup (64 or 256; 0 = 256 when there is a BVH top to share)
    int stack_pad = 0;                      // test hook: extra (unused) entries per traversal stack, to reach the > 64 KiB LDS launch path
    int radiance_persist = -1;              // urt_radiance_query: -1 = auto, 0 = one query per thread (k_radiance), 1 = resident grid + work counter (k_radiance_persist)
    int shade_min = 32, sky_min = 32;       // kernel_mode 3
    int serve_refill = 16;                  // kernel_mode 5: idle lanes of the traversal service that trigger a claim of waiting rays
    int front_list = -1;                    // kernel_mode 3: listed FRONT for scenes of <= 12 MeshObjects (-1 auto = on, 0 off)
    int shade_split = -1;                   // kernel_mode 3: -1 = auto (= split: measured better or equal on C2-C5), 0 = surface hits and misses shaded in one trip
    int front_fuse = -1;                    // kernel_mode 3, plain FRONT (one mesh, or "front_list" 0): -1 = auto (= on), 1 = a new ray takes its first object-level step in the trip that
                                            // created it, 0 = it waits for a voted FRONT trip (A/B and tests: both schedules in one build; same pixels)
    int handout = -1;                       // kernel_mode 3: how dead lanes get their pixel slots: 0 = every wave draws from its shard's counter (one device-scope atomic per refill),
                                            // 1 = the waves of a workgroup share a reservation of up to 16 tiles in LDS (one device-scope atomic per reservation), -1 = auto (= 1);
                                            // any value draws the same pixels (frame_device.h wg_fetch_pixels)
    int tile_order = -1;                    // persistent modes: order in which the frame's tiles are handed out: 0 bottom strip first, 1 top strip first (a launch then ENDS with the
                                            // bottom rows), -1 = auto: top first for scenes without triangle meshes (C2: -3.6 % in bench.py, -9 .. -12 % for launches of 1 - 20 frames),
                                            // bottom first otherwise (C3, driver's 20-frame launch: top first +1.5 %; 64-frame launches, C3D, C4, C5: +-0.4 %) —
                                            // profiles/r03_logs/r3_probe_tile_order.log; any order draws the same pixels
    int lds_tlas = 1;                       // kernel_mode 3: object-level heaps, roots and spheres in LDS when small
    int top_front = -1;                     // kernel_mode 3: top-of-forest walk inside the object-level phase (-1 = when the scene has several meshes)
    int top_nodes = -1;                     // kernel_mode 3: triangle-BVH nodes kept in LDS (0 = none; -1 = auto: 64, or with the masked object-level phase twice the number of
                                            // MeshObjects that have a BVH, rounded up to a power of two — there the top is walked lane by lane inside that phase and only its first level pays)
    int blas_builder = -1;                  // -1 = auto (default): 0 below kGpuBuildTriangles triangles, 3 from there on; 0 = binned SAH on host threads, 1 = Karras radix tree built on the GPU,
                                            // 2 = the same tree built top-down within a depth budget, 3 = binned SAH on the GPU (csrc/lbvh.hip): the host's trees at a fifth of the time on big scenes
    int frames_per_launch = 0;              // 0 = auto (own stream: 64 frames per launch, fewer when the Result slots would exceed 8 GiB; caller's stream: 1), 1 = off, 2..64
    int watchdog_cap = 0;                   // test hook: scheduler trips per wave (0 = auto, scaled with the launch)
    int lbvh_slack = 6;                     // blas_builder 2: levels of slack in the depth budget (csrc/lbvh.hip k_td_level)
    int front_cull = 1;                     // object-level cull (urt_math.h tlas_cull; csrc/cullflags.hip): 0 = every popped object is intersected, as the reference does
    int overlap_launches = 1;               // see "Overlapped launches" below
    int blas_cones = -1;                    // normal cones per triangle-BVH child (csrc/cones.hip): the scheduled kernel skips children whose triangles the ray sees from behind.
                                            // -1 = auto (= on), 0 = off (the words stay 0), 1 = on
    int tile_entry = -1;                    // kernel_mode 3, one MeshObject and no spheres: camera rays start their triangle-BVH walk at per-tile entry nodes (csrc/tile_entry.h)
                                            // while every frame of a launch has the same camera.  -1 = auto: on once the camera has stood still (a launch of >= 2 frames, or
                                            // the camera of the previous launch), 0 = off, 1 = on for every such launch; same pixels
  } opt;

  // ---- derived device scene ---------------------------------------------------------------------------------------------
  bool scene_dirty = true;
  // what made it dirty: SetData on a bound buffer sets the slot's bit; anything else (binding changes, options) asks for a full
  // preparation.  When only _MeshObjects / _MeshBVH / _Spheres / _SphereBVH contents changed, the scene is updated in place
  // (prepare_incremental: moved MeshObjects are refitted on the GPU, csrc/refit.hip)
  unsigned int dirty_slots = 0;
  bool dirty_full = true;
  // Everything that belongs to ONE prepared scene: free_scene frees scene_allocs and assigns Scene{}.
  struct Scene {
    urtd::DevScene ds{};
    std::vector<urtd::DeviceBuf<char>> scene_allocs;
    struct RefitAux {                       // device-resident (scene_allocs)
      const float* vertices = nullptr; const int32_t* indices = nullptr;      // copies of _Vertices / _Indices
      const float* normals = nullptr;         // copy of _Normals (null when the scene has none)
      int32_t* renormed = nullptr;            // per MeshObject: its shading normals are re-gathered by this update
      double* cost_base = nullptr; double* cost_now = nullptr;   // per MeshObject (cost sum, root area): at the full preparation / now (csrc/refit.hip tree_cost)
      int32_t* parent = nullptr; int32_t* node_mesh = nullptr; int32_t* depth = nullptr;
      float4* cbox = nullptr; unsigned int* ext = nullptr;
      float* matrices = nullptr; int32_t* moved = nullptr;
      bool ready = false;
    } refit;
    float4* qbuf = nullptr;                 // frame + quantized nodes (in scene_allocs)
    float4* cbuf = nullptr;                 // centre / half-extent copy of the nodes (in scene_allocs): DevScene::blas_cnodes
    float qnode_quality = 0;                // smallest MeshObject extent in grid cells (csrc/qnodes.hip)
    int4* cone_rng[2] = {nullptr, nullptr}; // option "blas_cones": the triangle range below every child and the relaxation's second buffer (in scene_allocs)
    const int4* cone_ranges = nullptr;      // the one of the two that holds the ranges, once they are found (csrc/cones.hip cone_ranges)
    bool cones_in_use = false;              // the cone words of cbuf are filled in (else they are 0)
    // urt_render_aov: one float4 per material in the order of DevScene::materials (pack_albedo), in scene_allocs.
    // Not a DevScene member: DevScene is an argument of every frame kernel, and the camera-matrix loads of k_sched depend on its size
    const float4* aov_albedo = nullptr;
    size_t cap_materials = 0, cap_mesh_tlas = 0, cap_sphere_tlas = 0, cap_sphere_pr = 0, cap_aov_albedo = 0;   // float4 capacities of the arrays updated in place
    int32_t* d_mesh_leaf = nullptr;         // per MeshObject: its heap leaf, or < 0 (in scene_allocs)
    size_t cap_mesh_leaf = 0;
    int walk_f4 = 0;                        // float4s of the masked-walk table behind the mesh heap's device copy (0 = none: heap > 31 nodes)
    int n_blas_nodes = 0;                   // interior nodes of the triangle-BVH forest (all meshes)
    int n_scene_tris = 0;                   // triangles of the prepared scene
    int scene_max_depth = 0;
    int tlas_stack = 2, blas_stack = 2;
    unsigned int watchdog_steps = 1u << 16;
    std::vector<int32_t> h_mesh_root, h_small_first;
    std::vector<int32_t> h_vert_lo, h_vert_hi;   // per MeshObject: the smallest and largest vertex its index range refers to (lo > hi: none)
    int n_vertices = 0, n_normals = 0;      // elements of _Vertices / _Normals the scene was prepared from
    std::vector<float> h_cost_base;         // per MeshObject: tree cost at the full preparation (read back at the first need)
    std::vector<uint8_t> prev_mesh_objects; // the _MeshObjects records the scene was prepared from
  } scene;
  // These outlive a scene:
  uint64_t scene_epoch = 0;                 // bumps at every scene preparation
  float last_prepare_ms = 0;                // host wall time of the last scene preparation (buffers -> device scene)
  int last_builder = 0;                     // the triangle-BVH builder the last full preparation of a scene WITH MeshObjects used (0..3): one without leaves it as it was
  uint64_t refitted_meshes = 0, incremental_preps = 0;
  uint64_t deformed_meshes = 0, renormed_meshes = 0, deform_bytes = 0, forced_rebuilds = 0;   // urt_debug_deform_stats
  float last_cost_ratio = 0;                // largest cost / baseline among the deformed MeshObjects of the last in-place update
  uint64_t full_preps = 0, device_preps = 0; // full preparations completed; those of them that option "prepare_device" fed from device memory (urt_debug_prepare_stats)
  float last_span_ms = 0;                   // option "time_dispatch": device time of the last vertex-span pass of a device-fed preparation (csrc/index_span.hip), else 0
  urtd::BlasCache blas_cache;               // per-MeshObject BVHs of the previous scene (reused when a MeshObject is unchanged)
  uint64_t nodes_epoch = 0;                 // bumps whenever the nodes the trace kernels read are rewritten (scene_prep.cpp rederive_nodes): builds, refits, cones
  // The tile entry table (csrc/tile_entry.h, option "tile_entry"): one table, for the camera, image size and node contents of `te_key`; a launch
  // with another key rebuilds it on its stream, behind the launches that still read it.  te_ready orders the build before launches on the other
  // streams; te_used[s] is recorded behind the last launch that read the table on stream s (0 the main stream, 1 / 2 the trace streams).
  struct TileEntryKey { float c2w[16], invp[16]; int width, height; uint64_t scene_epoch, nodes_epoch; const void* nodes; };
  urtd::DeviceBuf<int32_t> te_table;
  TileEntryKey te_key{}, te_seen_key{};     // the table's; the previous qualifying launch's (auto builds a table for a camera that stood still)
  bool te_valid = false, te_seen = false;
  hipStream_t te_stream = nullptr;          // the stream the table was built on
  urtd::Event te_ready, te_used[3];
  bool te_used_set[3] = {false, false, false};
  uint64_t te_builds = 0;                   // tables built since the context was created (urt_debug_read_tile_entry)
  int sched_groups = 0;                     // kernel_mode 3: workgroups per CU the last configuration counts on when fewer than the default fit (0 = default)
  urtd::DeviceBuf<float4> zero_sky;

  // wavefront queues
  urtd::PathQueues q{};                     // views of q_store / q_counts
  urtd::DeviceBuf<float4> q_store[2][4];
  urtd::DeviceBuf<unsigned int> q_counts;

  urtd::DeviceBuf<urtd::DevCounters> d_counters;   // kCounterShards shards
  // d_next / d_next2: the work-counter shards, then the diagnostic stamps (URT_STAMPS builds)
  static constexpr size_t kStampOffset = urtd::kWorkShards * 128, kStampBytes = 65536 * 16 * sizeof(unsigned long long), kWorkCounterBytes = kStampOffset + kStampBytes;
  urtd::DeviceBuf<unsigned int> d_next;     // persistent mode: frame work counter
  urtd::DeviceBuf<float4> d_mail;           // kernel_mode 5: posted rays (2 float4 per thread of the resident grid)
  // frame tables of the batched launches: kTableSlots pinned host images + device copies, used round-robin; a slot is reused
  // once the copy of its previous use has left the host image (event)
  static constexpr int kTableSlots = 4;
  static constexpr int kTableSlotEntries = urtd::kMaxFramesPerLaunch + 1;   // a launch's entries and, behind the last, 8 bytes: the address of its tile entry table
  urtd::PinnedBuf<urtd::FrameEntry> h_tables; urtd::DeviceBuf<urtd::FrameEntry> d_tables;
  urtd::Event table_ev[kTableSlots];
  unsigned int table_next = 0;
  uint64_t pixels_dispatched = 0;
  int n_cus = 256;

  uint64_t dispatches = 0;
  std::vector<std::pair<urtd::Event, urtd::Event>> timing;   // unresolved event pairs
  float trace_ms = 0;

  // ---- frame batching (kernel_mode 3) --------------------------------------------------------------------------------
  // A 1080p frame is small for this chip: ~40 % of its kernel time is the drain of the last long paths.
  // So dispatches are DEFERRED: consecutive frames that differ only in their per-frame uniforms (camera, _PixelOffset,
  // _Seed) are collected and traced by ONE persistent launch whose lanes move on to the next frame's pixels as soon as
  // the current frame is handed out.  Each frame's Result goes to its own slot of a slab (the Result texture is renamed
  // per dispatch), the AdditionShader blits that follow the dispatches are deferred with them and run in order after the
  // launch.  Everything else that could observe the images flushes first, so the in-order semantics of RM:806-820
  // stay exactly observable.
  // An operation deferred behind the batch's frames (flush_pending runs them in program order): urt_blit_add(src@frame -> dst, sample),
  // urt_blit_add_history(src@frame -> dst, count, max_history), urt_blit(src -> dst) — the present of RM:819 —, urt_texture_pack_rows[_rgb]
  // (src -> dense).  `frame`: the batch's last frame when it was queued, the slot `src` names when it is the batch's Result texture.
  enum class OpKind { BlendAdd, BlendHistory, Copy, PackRows };
  struct PostOp {
    OpKind kind;
    int frame;
    urt_handle src = 0, dst = 0;
    float sample = 0;                                                             // BlendAdd
    urt_handle count = 0; float max_history = 0;                                  // BlendHistory
    void* dense = nullptr; int first_row = 0, row_stride = 1; bool rgb = false;   // PackRows
    bool touches(urt_handle t) const { return src == t || dst == t || count == t; }
  };
  struct Pending {
    int n = 0, limit = 1;
    urt_handle tex = 0;                     // the Result texture of the batch
    uint64_t scene_epoch = 0;
    urtd::DevScene S{};
    urtd::FrameParams P{};                  // frame 0's; the frames agree on everything but the table entries
    urtd::FrameTable T{};
    int front_mode = 0; bool count = false;
    std::vector<PostOp> ops;
  } pend;
  urtd::DeviceBuf<float4> slab;             // slab_frames x slab_stride float4: Result slots of the batched frames
  size_t slab_stride = 0;
  int slab_frames = 0;
  urt_handle slab_tex = 0;                  // the texture whose `dev` may point into the slab
  int slab_frames_max = 0;                  // largest batch the Result slab could be allocated for (after out-of-memory retries)
  size_t slab_oom_stride = 0;               // image size (pixels) for which not even two slots could be allocated
  std::vector<urtd::Event> event_pool;      // recycled timing events
  urtd::Event ev_switch;                    // orders the old stream before the new one in urt_context_set_stream
  uint64_t launches = 0;                    // trace-kernel launches (a batched launch counts once)
  urt_launch_info last_launch{};            // the last trace launch of this context (urt_debug_launch_info)
  // a wave that left a persistent kernel through one of its caps has not written its pixels: the kernels raise this host-mapped
  // word (frame_device.h report_watchdog) and the next synchronising call fails with URT_ERR_WATCHDOG
  urtd::PinnedBuf<unsigned int> h_trip_flag;   // pinned, device-visible
  unsigned int* d_trip_flag = nullptr;      // its device address
  // Overlapped launches (option "overlap_launches", flush_pending): a host that SUBMITS every frame (urt_flush, a present into an external
  // texture) produces one-frame launches, and a one-frame launch is mostly ramp and drain.  Small launches therefore alternate between two trace streams and take their Result slots
  // round-robin from the slab, so that launch L+1 fills the wave slots launch L's draining waves give back; the blends / presents /
  // readbacks stay on the main stream, in program order, each behind its own launch.
  static constexpr int kOverlapFrames = 8;  // launches of up to this many frames take part
  urtd::Stream trace_q[2];
  urtd::Event trace_done[2], pre_ev[2], dep_ev;
  urtd::DeviceBuf<unsigned int> d_next2;    // the second launch in flight needs work counters of its own
  unsigned int trace_parity = 0;
  bool main_touched = true;                 // something other than the frame loop's own blends / presents / readbacks was enqueued on the main stream since the last launch
  int slab_cursor = 0, prev_base = 0, prev_n = 0;
  std::vector<const float4*> prev_writes;   // the device images the deferred blends / copies / presents of the last submission write: the narrow dependency does not cover them
  uint64_t overlapped_launches = 0;

  // pipelined readback (urt_texture_read_begin / _end): kReadSlots snapshots in flight, each a device copy + a pinned host image
  static constexpr int kReadSlots = 3;
  struct ReadSlot { urtd::DeviceBuf<float4> dev; urtd::PinnedBuf<float4> host; size_t bytes = 0; int format = 0; urtd::Event snap, done; bool busy = false; uint64_t ticket = 0; } rslot[kReadSlots];
  urtd::DeviceBuf<float> srgb_first;          // device: first float of every 8-bit sRGB code (csrc/present.hip), made at the first RGBA8 readback
  urtd::Stream copy_stream;
  uint64_t read_next = 0;

  // Grow-only device scratch (owned.h reserve) of the calls that take host memory or need room of their own:
  urtd::DeviceBuf<urt_Ray> q_rays; urtd::DeviceBuf<urt_RayHit> q_out;   // urt_ray_query: the rays and the results
  urtd::DeviceBuf<char> rq_in; urtd::DeviceBuf<float4> rq_out;          // urt_radiance_query: the queries (bytes) and the results (texels)
  urtd::DeviceBuf<unsigned int> rq_next;      // the work counter of k_radiance_persist (one word; each launch zeroes it on the stream in front of itself)
  urtd::DeviceBuf<float4> dn_scratch;         // urt_denoise: 3 images (guide, two colour images)
  urtd::DeviceBuf<urt_ObjectMotion> mo_table[2];   // urt_reproject_objects: copies of the mesh and the sphere motion table
  // urt_select_pixels / urt_resample_below: the per-block counts and the total behind them, and a pinned host word the total is copied to;
  // urt_resample_below: the pixel list and its samples, both sized by the selected count, not by the image
  urtd::DeviceBuf<unsigned int> rs_counts; urtd::PinnedBuf<unsigned int> rs_total;
  urtd::DeviceBuf<urt_PathPixel> rs_pixels; urtd::DeviceBuf<float4> rs_samples;
  urtd::DeviceBuf<unsigned int> ex_accum;     // urt_auto_exposure: the histogram's accumulators (csrc/tonemap.h), zero whenever no call is in flight
  urtd::DeviceBuf<float4> bl_pyramid;         // urt_bloom: the levels 1..L of the largest call so far, back to back (csrc/bloom.h); every call writes what it reads
  urtd::DeviceBuf<float> df_scratch;          // urt_depth_of_field: {a, z} per pixel and the tile table of the largest call so far (csrc/dof.h); every call writes what it reads
  urtd::DeviceBuf<float> mb_scratch;          // urt_motion_blur: the tile table and {l, z} per pixel of the largest call so far (csrc/motion_blur.h); every call writes what it reads
  // Buffer mirrors (context.cpp): what a host SetData changed in a mirrored buffer travels through one of kUpSlots pinned images, used
  // round-robin; a slot is reused once the copy of its previous use has left it (event) — no wait for the stream's other work
  static constexpr int kUpSlots = 4;
  struct UpSlot { urtd::PinnedBuf<char> host; urtd::Event done; bool used = false; } up_slot[kUpSlots];
  unsigned int up_next = 0;
  urtd::DeviceBuf<float> bd_partial; urtd::PinnedBuf<float> bd_result;   // urt_buffer_bounds: the per-block partials (and, behind them, the result); its host image
  urtd::DeviceBuf<float> ob_partial;          // urt_mesh_leaf_bounds_device: the per-block partials of the largest call so far (csrc/object_bvh.h)
  urtd::DeviceBuf<float4> nm_face;            // urt_compute_normals: the face normals of the largest plan so far, 16 bytes each
};

namespace urtd {

using PostOp = urt_context::PostOp;
using OpKind = urt_context::OpKind;

#define URT_HIP(ctx, expr)                                                                         \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail(ctx, e__ == hipErrorOutOfMemory ? URT_ERR_OUT_OF_MEMORY : URT_ERR_HIP,           \
                  std::string(#expr) + ": " + hipGetErrorString(e__));                            \
  } while (0)

#define URT_GUARD_BEGIN try {
#define URT_GUARD_END(ctx)                                                                         \
  } catch (const std::bad_alloc&) { return fail(ctx, URT_ERR_OUT_OF_MEMORY, "host allocation failed"); } \
  catch (const std::exception& ex) { return fail(ctx, URT_ERR_INVALID_ARGUMENT, ex.what()); }        \
  catch (...) { return fail(ctx, URT_ERR_INVALID_ARGUMENT, "unknown exception"); }

inline hipStream_t touch(urt_context* ctx) { ctx->main_touched = true; return ctx->stream; }

inline Texture* find_texture(urt_context* ctx, urt_handle h) {
  auto it = ctx->textures.find(h);
  return it == ctx->textures.end() ? nullptr : &it->second;
}

inline Buffer* find_buffer(urt_context* ctx, urt_handle h) {
  auto it = ctx->buffers.find(h);
  return it == ctx->buffers.end() ? nullptr : &it->second;
}

// The bound buffer of a slot, or null when it holds nothing.  Readers of `host` have called buffer_sync_host / sync_bound_hosts.
inline const Buffer* bound_buffer(urt_context* ctx, int slot) {
  urt_handle h = ctx->bound[slot];
  if (!h) return nullptr;
  auto it = ctx->buffers.find(h);
  if (it == ctx->buffers.end() || !it->second.has_data || it->second.count == 0) return nullptr;
  return &it->second;
}

// The camera uniforms bound now (RS:5-7, 16), as the kernels that draw camera rays outside a FrameParams take them
inline FrameUniforms bound_camera(const urt_context* ctx) {
  FrameUniforms C{};
  std::memcpy(C.c2w, ctx->c2w, sizeof C.c2w);
  std::memcpy(C.invp, ctx->invp, sizeof C.invp);
  C.pixel_off_x = ctx->pixel_off[0]; C.pixel_off_y = ctx->pixel_off[1];
  C.seed = ctx->seed;
  return C;
}

// LDS entries per lane of the prepared scene's two traversal stacks, for every kernel that traces one ray per lane; stack_pad is unused room
inline LaneStackSize lane_stack_size(const urt_context* ctx) { return {ctx->scene.tlas_stack, ctx->scene.blas_stack + ctx->opt.stack_pad}; }

inline int heap_levels(int n) { int l = 0; while (n > 0) { l++; n >>= 1; } return l; }   // floor(log2 n) + 1

// max_history of urt_reproject / urt_blit_add_history: 0 (unlimited) or >= 1
inline bool valid_max_history(float v) { return !std::isnan(v) && (v == 0.0f || v >= 1.0f); }

// context.cpp
int check_watchdog(urt_context* ctx);
int download_elements(urt_context* ctx, Buffer& b, int first, int last);   // mirror -> host, synchronising, counted
int buffer_sync_host(urt_context* ctx, Buffer& b);          // downloads the stale range (synchronises; counted), after which `host` is current
int sync_bound_hosts(urt_context* ctx, unsigned int slots); // ... of the buffers bound to the slots of the mask
int buffer_mirror(urt_context* ctx, Buffer& b);             // the device mirror, made and filled from `host` at the first need
int strip_count(int group_rows, int first_row, int row_stride);
void mark_device_written(urt_context* ctx, urt_handle buffer, Buffer& b, int first, int count);   // a kernel or copy has filled these elements (count > 0) of the mirror
int check_element_range(urt_context* ctx, const char* who, const Buffer& b, int first, int count);
// geometry_ops.cpp: the buffer arguments of a call that works on device mirrors, looked up as image_ops.cpp looks up its textures (TexArg)
struct BufArg { urt_handle h; const char* name; int stride; bool absent = false; };   // absent: not part of this call (no normals wanted), whatever h is
int resolve_buffers(urt_context* ctx, const char* who, const BufArg* a, int n, Buffer** b);   // b[k] = the buffer of a[k] (null: absent): every handle, then every stride, in argument order
int mirror_buffers(urt_context* ctx, Buffer* const* b, int n);   // buffer_mirror of every buffer given: after the last check, before anything is enqueued
// scene_prep.cpp
int prepare_scene(urt_context* ctx);
int scene_cost(urt_context* ctx, std::vector<float>& now, std::vector<float>& base);
void free_scene(urt_context* ctx);
bool build_walk_table(const Buffer* heap, int n_meshes, const std::vector<int32_t>& mesh_root, const std::vector<int32_t>& small_first,
                      std::vector<float>& out);
// frame_batch.cpp
int flush_pending(urt_context* ctx);
int do_dispatch(urt_context* ctx, int kernel, int gx, int gy, int gz, int first_row, int row_stride);
int bind_sky(urt_context* ctx, DevScene& S);
bool in_slab(urt_context* ctx, const Texture& t);
int detach_from_slab(urt_context* ctx, Texture& t);
int resolve_timing(urt_context* ctx);

// The scene the bound buffers describe: a stale one is prepared first, after the deferred frames that read the one it replaces.
inline int current_scene(urt_context* ctx) {
  if (!ctx->scene_dirty) return URT_OK;
  if (int rc = flush_pending(ctx)) return rc;
  return prepare_scene(ctx);
}

}  // namespace urtd
