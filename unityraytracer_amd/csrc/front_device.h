// front_device.h — the object-level phase of the phase-scheduled kernels (mode 3: kernels.hip k_sched, mode 5: kernels_serve.hip
// k_serve; mode 4 uses trace_front alone): Trace() cut at its triangle-BVH visits, in its plain, listed and masked forms, over the
// LDS copies of the object-level tables that the kernel's prologue makes (FrontLds, WalkLds; kernels.hip k_sched).
#pragma once
#include "frame_device.h"
#include "tile_entry.h"      // kTileEntryK: the record tile_entry_start reads

namespace {

// Trace() (RS:364-383) cut at its triangle-BVH visits, for the phase-scheduled kernels: runs from the start of Trace
// (`fresh`) or from the return of a triangle-BVH visit up to the NEXT MeshObject whose triangle BVH must be walked
// (returns true, `cur` = its root) or to the end of Trace (returns false; `best` is final).  `check`/`seen` are the
// object-level walk's stack height and its never-reset `tests` flag (RS:296-297, A.5); the object-level stack entry e of
// this path is tl[e * stride].
// TOPF (multi-mesh scenes): a ray entering a MeshObject walks the LDS-resident top of the forest (`top`, nodes
// [0, top_nodes)) right here, far children going on its traversal stack `bl` (height *sp_out): when nothing of the mesh is
// near the ray the heap walk simply continues — no round trip through the traversal phase for a mesh that is only grazed.
// FrontLds: LDS copies of the small object-level tables (null = read the global buffer).  An object-level walk is a chain
// of dependent fetches (C2: 19 heap nodes per ray); from LDS each costs tens of cycles instead of an L1/L2 round trip.
struct FrontLds {
  const float4* mesh_tlas = nullptr;     // [2 * n_mesh_tlas]
  const int32_t* mesh_root = nullptr;    // [n_meshes]
  const float4* sphere_tlas = nullptr;   // [2 * n_sphere_tlas]
  const float4* sphere_pr = nullptr;     // [n_spheres]
  const float4* small_tris = nullptr;    // [3 * n_small] triangle records of the single-leaf MeshObjects
  const int32_t* small_first = nullptr;  // [n_meshes] first triangle of MeshObject m in small_tris, or -1
};

// SP0: the height an empty triangle-BVH stack has for the caller (1 = a sentinel sits in entry 0: k_sched)
// CONES (with SP0 = 1 only: k_sched): the walk of the BVH top applies the normal-cone test (trace_device.h cone_skips)
template <bool COUNT, bool TOPF = false, bool RAYS = true, int SP0 = 0, bool CONES = false>
__device__ __forceinline__ bool trace_front(const DevScene& S, bool fresh, v3 o, v3 d, HitRec& best, int& check, bool& seen,
                                            int* tl, int stride, int32_t& cur, LocalCounters& lc, const FrontLds& L = FrontLds(),
                                            const float4* top = nullptr, int top_nodes = 0, int* bl = nullptr, int* sp_out = nullptr) {
  if (fresh) {
    if (RAYS) lc.rays++;                                    // (k_sched counts its rays per wave instead: one register less per lane)
    best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
    float t = -o.y / d.y;                                   // IntersectGroundPlane RS:156-172
    if (t > 0 && t < best.t) { best.t = t; best.kid = 1; }
    check = 0; seen = false;
    if (S.n_meshes > 0) { check = 1; tl[0] = 0; }
  }
  v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
  // the object-level cull (urt_math.h tlas_cull) compares with the ground-plane hit distance; the walk resumes after triangle-BVH visits that
  // have changed best.t, so that distance is re-derived where a leaf with a cull word is met (the same operations as RS:156-172 above — and
  // only there: kept live across the loop it cost 32 B/lane of scratch in the single-mesh instantiation)
  const bool may_cull = S.cull_any != 0;
  while (check > 0) {                                        // IntersectMeshBVH RS:294-326
    check--;
    int bi = tl[check * stride];
    bool hit = false; int index = -1;
    float t_min = 0.0f, t_max = 0.0f; int cull_word = 0;
    if (bi < S.n_mesh_tlas) {
      if (COUNT) lc.tlas_nodes++;
      float4 a, b;
      if (L.mesh_tlas) { a = L.mesh_tlas[2 * bi]; b = L.mesh_tlas[2 * bi + 1]; } else { a = S.mesh_tlas[2 * bi]; b = S.mesh_tlas[2 * bi + 1]; }
      index = as_int(a.w);
      if (may_cull) { hit = tlas_slab_t(a, b, o, rcp, t_min, t_max); cull_word = as_int(b.w); }
      else hit = tlas_slab(a, b, o, rcp);
    }
    if (hit) {
      if (index < 0) { tl[check * stride] = bi * 2 + 1; check++; tl[check * stride] = bi * 2 + 2; check++; }
      else seen = true;
    }
    bool culled = false;
    if (cull_word != 0) { float t = -o.y / d.y; culled = tlas_cull(t_min, t_max, t > 0 ? t : URT_INF); }      // (the ground-plane hit distance, re-derived: RS:156-172)
    if (seen && !culled && index >= 0 && index < S.n_meshes) {
      int32_t root;
      if (L.mesh_root) root = L.mesh_root[index]; else root = S.mesh_root[index];
      if (root < 0 && root != kBlasDone) {               // a mesh of <= 8 triangles is one leaf: test it here, no phase switch
        int bi_local = -1;
        if (L.small_tris) test_leaf<COUNT>(S, root, o, d, best, bi_local, lc, L.small_tris, L.small_first[index]);
        else test_leaf<COUNT>(S, root, o, d, best, bi_local, lc);
      } else if (root != kEmptyMeshRoot) {
        if (TOPF) {
          int sp = SP0;
          if (root < top_nodes) {
            BlasRay R = blas_ray(o, d);    // recomputed per MeshObject entered: keeping it live across the heap walk costs more (spills)
            if (SP0 == 1) root = blas_walk_top_ptr<COUNT, CONES>(top, top_nodes, root, R, best.t, bl, sp, lc, CONES ? cone_ray_word(d) : 0);
            else do root = blas_node_step_top<COUNT>(top, root, R, best.t, bl, sp, lc); while (root >= 0 && root < top_nodes);
          }
          *sp_out = sp;
          if (root == kBlasDone) continue;                   // nothing of this mesh is near the ray: on with the heap walk
        }
        cur = root;
        return true;
      }
    }
  }
  if (S.n_spheres > 0) {                                   // IntersectSphereBVH RS:329-361
    int c2 = 1; tl[0] = 0; bool seen2 = false;
    while (c2 > 0) {
      c2--;
      int bi = tl[c2 * stride];
      bool hit = false; int index = -1;
      if (bi < S.n_sphere_tlas) {
        if (COUNT) lc.tlas_nodes++;
        float4 a, b;
        if (L.sphere_tlas) { a = L.sphere_tlas[2 * bi]; b = L.sphere_tlas[2 * bi + 1]; } else { a = S.sphere_tlas[2 * bi]; b = S.sphere_tlas[2 * bi + 1]; }
        index = as_int(a.w);
        hit = tlas_slab(a, b, o, rcp);
      }
      if (hit) {
        if (index < 0) { tl[c2 * stride] = bi * 2 + 1; c2++; tl[c2 * stride] = bi * 2 + 2; c2++; }
        else seen2 = true;
      }
      if (seen2 && index >= 0 && index < S.n_spheres) intersect_sphere<COUNT>(S, index, o, d, best, lc, L.sphere_pr);
    }
  }
  return false;
}

// The fresh step of trace_front<COUNT, false> for a scene whose mesh heap is ONE node and that has no spheres (C3: one MeshObject), written
// straight: the ground plane, the three reciprocals, the slab test of node 0, its cull decision, the root lookup — the operations of the
// loop's only iteration that does anything, in its order, without the loop, the object-level stack or the `check` / `seen` state.  (A
// node that is no leaf pushes children 1 and 2, which lie past the heap and pop as nothing: the walk ends with nothing seen, here too.)
// `cs` leaves as the loop would have left it: height 0, the `tests` flag << 8.  The ground-plane distance that the cull compares with is
// the one computed two lines above — the same division of the same operands that the loop repeats at the leaf.
template <bool COUNT>
__device__ __forceinline__ bool front_single(const DevScene& S, v3 o, v3 d, HitRec& best, int& cs, int32_t& cur, LocalCounters& lc, const FrontLds& L) {
  best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
  float t = -o.y / d.y;                                     // IntersectGroundPlane RS:156-172
  if (t > 0 && t < best.t) { best.t = t; best.kid = 1; }
  v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
  if (COUNT) lc.tlas_nodes++;
  float4 a, b;
  if (L.mesh_tlas) { a = L.mesh_tlas[0]; b = L.mesh_tlas[1]; } else { a = S.mesh_tlas[0]; b = S.mesh_tlas[1]; }
  const int index = as_int(a.w);
  bool hit; float t_min = 0.0f, t_max = 0.0f; int cull_word = 0;
  if (S.cull_any != 0) { hit = tlas_slab_t(a, b, o, rcp, t_min, t_max); cull_word = as_int(b.w); }
  else hit = tlas_slab(a, b, o, rcp);
  const bool seen = hit && index >= 0;
  cs = seen ? 256 : 0;
  bool culled = false;
  if (cull_word != 0) culled = tlas_cull(t_min, t_max, t > 0 ? t : URT_INF);
  if (seen && !culled && index < S.n_meshes) {
    int32_t root;
    if (L.mesh_root) root = L.mesh_root[index]; else root = S.mesh_root[index];
    if (root < 0 && root != kBlasDone) {                    // a mesh of <= 8 triangles is one leaf: tested here
      int bi_local = -1;
      if (L.small_tris) test_leaf<COUNT>(S, root, o, d, best, bi_local, lc, L.small_tris, L.small_first[index]);
      else test_leaf<COUNT>(S, root, o, d, best, bi_local, lc);
    } else if (root != kEmptyMeshRoot) {
      cur = root;
      return true;
    }
  }
  return false;
}

// A camera ray that front_single sends into the mesh's triangle BVH starts at its tile's entries instead of the root (tile_entry.h:
// the pre-pass has walked what all rays of the 8x8 tile have in common and dropped the children none of them can enter or keep).
// `te`: the table, 8 dwords per tile of the whole image (width pixels wide), row by row: word 0 = the first node, words 1 .. 7 = the
// stack above the sentinel, bottom first, padded with kBlasDone.  All 7 go to the lane's stack — the launcher guarantees that many
// entries, and what lies above the height is free room —, the height counts the ones that are entries.  Returns false for an empty
// list: nothing of the mesh is near any ray of the tile.  The walk that follows is the usual one: the same node steps, leaf tests and
// tie rule on every triangle the ray can hit, so the winner is the same.
static_assert(kTileEntryK == 8 && kTileEntryDone == kBlasDone, "tile_entry_start reads two int4 per tile");
// the table's address: two dwords behind the launch's last frame entry (kernels.h launch_sched), read with scalar loads where it is used
__device__ __forceinline__ const int4* launch_tile_entry_table(const FrameEntry* T, int n_frames) {
  typedef const __attribute__((address_space(4))) unsigned int* kuintp;
  kuintp p = (kuintp)(unsigned long long)(T + __builtin_amdgcn_readfirstlane(n_frames));
  asm volatile("" : "+s"(p));                      // opaque to LICM: the load stays at its use, not in two scalar registers across the trace loop
  return (const int4*)(((unsigned long long)p[1] << 32) | (unsigned long long)p[0]);
}
__device__ __forceinline__ bool tile_entry_start(const int4* __restrict__ te, int width, int xy, int* bl, int32_t& cur, int& sp) {
  const unsigned int tiles_w = ((unsigned int)width + 7u) >> 3;
  const int4* rec = te + 2u * (((unsigned int)xy >> 19) * tiles_w + (((unsigned int)xy & 0xffffu) >> 3));
  const int4 a = rec[0], b = rec[1];
  cur = a.x;
  bl[64] = a.y; bl[128] = a.z; bl[192] = a.w; bl[256] = b.x; bl[320] = b.y; bl[384] = b.z; bl[448] = b.w;
  sp = 1 + (a.y != kBlasDone) + (a.z != kBlasDone) + (a.w != kBlasDone) + (b.x != kBlasDone) + (b.y != kBlasDone) + (b.z != kBlasDone) + (b.w != kBlasDone);
  return a.x != kBlasDone;
}

// FRONT for multi-mesh scenes, "listed" form (front mode 2). In trace_front<TOPF> the expensive bodies — the inline triangle tests
// of single-leaf MeshObjects (wall quads: ~150 VALU) and the walk of the LDS-resident top of a big MeshObject's BVH (~60 + 50 per
// node) — sit INSIDE the per-lane heap-walk loop: every iteration of that loop pays for both whenever any lane of the wave
// happens to be at such a leaf.  The object-level slab test (RS:271-291) never looks at the best hit so far, so WHICH objects a ray
// tests, and in which order, is a function of the ray and the heap alone.  Here a fresh ray first walks the whole heap (cheap:
// ~30 VALU per node) and writes the object ids it has to test, in the reference's order (pop order, `tests` never reset: A.5),
// as bytes into its LDS column; then the wave works the lists off in two alternating bodies: the inline triangle tests for every
// lane whose next entry is a single-leaf MeshObject, until all lanes stand at a big one, then ONE BVH-top walk for all of
// them.  Every lane still tests its objects in list order, so ties in t resolve exactly as before.  A lane whose ray has to enter a MeshObject's BVH below the LDS top leaves for the
// BLAS phase and resumes with its next entry.  cs = entries left | next entry << 8.  Called by the whole wave (`mine` = lanes in
// FRONT / RESUME); needs the object-level mesh tables in LDS and n_meshes <= 12.
// The list: up to 12 object ids of 5 bits, six per dword, kept in two registers during the walk and then in the first two
// entries of the lane's object-level stack column — the stack is dead once the walk is over, so the list costs no LDS at all
// (LDS is what limits the size of the BVH top a workgroup can keep: a first version with a byte list of its own shrank that top
// and tripled the time spent in the BLAS phase).
__device__ __forceinline__ int list_get(const int* tl, int j) {
  unsigned int w = (unsigned int)tl[j >= 6 ? 64 : 0];
  return (int)((w >> (5 * (j >= 6 ? j - 6 : j))) & 31u);
}

// Returns per lane: 0 = Trace() is complete (shade next), 1 = the ray must enter a triangle BVH (BLAS phase next), 2 = not served in this
// trip (a fresh ray whose heap walk was put off: fresh rays walk the heap together, when at least 16 of them wait or when no
// resumed ray needs the trip — resumed rays are the majority in scenes where a ray meets several big meshes, and a walk for a
// few fresh lanes would hold all of them up).
#ifdef URT_STAMPS
#define URT_FS_DECL , unsigned long long* fs
#define URT_FS_ARG , fs_arr
#define URT_FS(stmt) stmt
#else
#define URT_FS_DECL
#define URT_FS_ARG
#define URT_FS(stmt)
#endif
template <bool COUNT, int SP0 = 0, bool CONES = false>
__device__ __forceinline__ int front_listed(const DevScene& S, const FrameParams& P, bool mine, bool fresh, v3 o, v3 d, HitRec& best, int& cs,
                                            int* tl, int32_t& cur, LocalCounters& lc, const FrontLds& L, const float4* top, int* bl, int& sp,
                                            unsigned int& wave_rays URT_FS_DECL) {
  URT_FS(unsigned long long fs_t0 = wall_clock64();)
  int remaining = cs & 0xff, cursor = cs >> 8;
  const int n_fresh = __popcll(wballot(mine && fresh)), n_resumed = __popcll(wballot(mine && !fresh));
  const bool walk_now = n_fresh >= 16 || n_resumed == 0;
  if (!walk_now) mine = mine && !fresh;
  else wave_rays += (unsigned int)n_fresh;                  // Trace() invocations (RS:454), counted per wave
  const bool put_off = !walk_now && fresh;
  if (mine && fresh) {
    best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
    float t = -o.y / d.y;                                   // IntersectGroundPlane RS:156-172
    if (t > 0 && t < best.t) { best.t = t; best.kid = 1; }
    v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
    int count = 0, check = 0;
    unsigned int l0 = 0, l1 = 0;
    bool seen = false;
    if (S.n_meshes > 0) { check = 1; tl[0] = 0; }
    const float t_ground = best.t;                           // what the object-level cull compares with (urt_math.h tlas_cull)
    while (check > 0) {                                      // IntersectMeshBVH RS:294-326, the walk alone
      check--;
      int bi = tl[check * 64];
      bool hit = false, culled = false; int index = -1;
      if (bi < S.n_mesh_tlas) {
        if (COUNT) lc.tlas_nodes++;
        float4 a = L.mesh_tlas[2 * bi], b = L.mesh_tlas[2 * bi + 1];
        index = as_int(a.w);
        float t_min, t_max;
        hit = tlas_slab_t(a, b, o, rcp, t_min, t_max);
        culled = leaf_culled(b, t_min, t_max, t_ground);
      }
      if (hit) {
        if (index < 0) { tl[check * 64] = bi * 2 + 1; check++; tl[check * 64] = bi * 2 + 2; check++; }
        else seen = true;
      }
      if (seen && !culled && index >= 0 && index < S.n_meshes && L.mesh_root[index] != kEmptyMeshRoot) {
        if (count < 6) l0 |= (unsigned int)index << (5 * count); else l1 |= (unsigned int)index << (5 * (count - 6));
        count++;
      }
    }
    tl[0] = (int)l0; tl[64] = (int)l1;                       // the walk's stack is dead: its first two entries keep the list
    remaining = count; cursor = 0;
  }
  URT_FS(if (walk_now && n_fresh > 0) { fs[0] += wall_clock64() - fs_t0; fs[3]++; fs[6] += (unsigned long long)n_fresh; })
  bool need = false;
  bool has = mine && remaining > 0;
  for (;;) {
    // (1) every lane works off the single-leaf MeshObjects (<= 8 triangles: wall quads, planes) at the head of its list:
    //     one cheap body for all of them, until every lane's next entry is a big MeshObject (or its list is done)
    int obj = 0; int32_t root = kEmptyMeshRoot;
    URT_FS(unsigned long long fs_t1 = wall_clock64();)
    for (;;) {
      if (has) { obj = list_get(tl, cursor); root = L.mesh_root[obj]; }
      bool small = has && root < 0;
      if (wballot(small) == 0) break;
      URT_FS(fs[4]++;)
      if (small) {
        int bi_local = -1;
        if (L.small_tris) test_leaf<COUNT>(S, root, o, d, best, bi_local, lc, L.small_tris, L.small_first[obj]);
        else test_leaf<COUNT>(S, root, o, d, best, bi_local, lc);
        cursor++; remaining--; has = remaining > 0;
      }
    }
    // (2) ONE walk of the LDS-resident BVH top for all the lanes that now stand at a big MeshObject: the expensive body runs with
    //     as many lanes as the wave can muster, as often as the longest list has big entries
    URT_FS(fs[1] += wall_clock64() - fs_t1; fs_t1 = wall_clock64();)
    if (wballot(has) == 0) break;
    URT_FS(fs[5]++;)
    if (has) {
      sp = SP0;
      if (root < P.top_nodes) {
        BlasRay R = blas_ray(o, d);
        if (SP0 == 1) root = blas_walk_top_ptr<COUNT, CONES>(top, P.top_nodes, root, R, best.t, bl, sp, lc, CONES ? cone_ray_word(d) : 0);
        else do root = blas_node_step_top<COUNT>(top, root, R, best.t, bl, sp, lc); while (root >= 0 && root < P.top_nodes);
      }
      cursor++; remaining--;
      if (root == kBlasDone) has = remaining > 0;           // nothing of this mesh is near the ray
      else { cur = root; need = true; has = false; }         // on to the BLAS phase; the list continues at RESUME
    }
    URT_FS(fs[2] += wall_clock64() - fs_t1;)
  }
  cs = remaining | (cursor << 8);
  if (mine && !need && S.n_spheres > 0) {                    // IntersectSphereBVH RS:329-361
    v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
    int c2 = 1; tl[0] = 0; bool seen2 = false;
    while (c2 > 0) {
      c2--;
      int bi = tl[c2 * 64];
      bool hit = false; int index = -1;
      if (bi < S.n_sphere_tlas) {
        if (COUNT) lc.tlas_nodes++;
        float4 a, b;
        if (L.sphere_tlas) { a = L.sphere_tlas[2 * bi]; b = L.sphere_tlas[2 * bi + 1]; } else { a = S.sphere_tlas[2 * bi]; b = S.sphere_tlas[2 * bi + 1]; }
        index = as_int(a.w);
        hit = tlas_slab(a, b, o, rcp);
      }
      if (hit) {
        if (index < 0) { tl[c2 * 64] = bi * 2 + 1; c2++; tl[c2 * 64] = bi * 2 + 2; c2++; }
        else seen2 = true;
      }
      if (seen2 && index >= 0 && index < S.n_spheres) intersect_sphere<COUNT>(S, index, o, d, best, lc, L.sphere_pr);
    }
  }
  return put_off ? 2 : need ? 1 : 0;
}

// FRONT for multi-mesh scenes, "masked" form (front mode 3): front_listed without the divergent heap walk and without the list.
// For a mesh heap of <= 31 nodes the object-level walk (RS:294-326) is a function of one bit per node — did the ray pass the node's
// slab test (RS:271-291; it never looks at the best hit so far) — and of the heap's static shape.  The nodes are kept in POP
// order (right-first pre-order: children are pushed 2i+1 then 2i+2, so the right child is popped first): the right child of the
// node at position p sits at p + 1, the left child at p + 2^(levels below p).  A fresh ray evaluates the slab test of every node
// whose outcome can matter (wave-uniform loop, bounds broadcast from LDS, no stack, no divergence), then derives with a few
// mask operations
//     P = popped nodes: the root, and level by level the children of popped, hit, interior nodes (two shifts per level),
//     T = the MeshObjects to test: popped leaves from the first popped-AND-hit leaf on in pop order (`tests` is never reset: A.5),
// and keeps T in one register: bit order = the reference's test order.  The wave then works the masks off exactly as front_listed
// works its lists off (inline triangle tests for lanes at a single-leaf MeshObject, one BVH-top walk for lanes at a big one).
// W = the walk table in LDS (scene_prep.cpp build_walk_table).  cs = T.  Returns 0 / 1 / 2 like front_listed.
struct WalkLds {
  const int* hdr = nullptr;            // [0] n_eval, levels, interior mask, exist mask  [4] leaf_any, leaf_valid  [8..11] depth masks  [12..15] left-child shifts
  const int* pos_tab = nullptr;        // [2p] triangle-BVH root of the object at position p, [2p+1] its first triangle in small_tris or -1
  const float4* eval = nullptr;        // [2e] vmin.xyz, position bit of the parent (0: the root)  [2e+1] vmax.xyz, position bit
};
template <bool COUNT, int SP0 = 0, bool CONES = false>
__device__ __forceinline__ int front_masked(const DevScene& S, const FrameParams& P, bool mine, bool fresh, v3 o, v3 d, HitRec& best, int& cs,
                                            int* tl, int32_t& cur, LocalCounters& lc, const FrontLds& L, const WalkLds& W, const float4* top, int* bl, int& sp,
                                            unsigned int& wave_rays URT_FS_DECL) {
  URT_FS(unsigned long long fs_t0 = wall_clock64();)
  unsigned int T = (unsigned int)cs;
  const int n_fresh = __popcll(wballot(mine && fresh)), n_resumed = __popcll(wballot(mine && !fresh));
  const bool walk_now = n_fresh >= 16 || n_resumed == 0;
  if (!walk_now) mine = mine && !fresh;
  else wave_rays += (unsigned int)n_fresh;                  // Trace() invocations (RS:454), counted per wave
  const bool put_off = !walk_now && fresh;
  if (walk_now && n_fresh > 0) {                             // (wave-uniform: the loop below runs on scalar control flow)
    const bool walker = mine && fresh;
    if (walker) {
      best.t = URT_INF; best.kid = 0; best.u = 0; best.v = 0;
      float t = -o.y / d.y;                                 // IntersectGroundPlane RS:156-172
      if (t > 0 && t < best.t) { best.t = t; best.kid = 1; }
    }
    v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
    unsigned int H = 0, Cm = 0;                              // slab test passed; object culled (urt_math.h tlas_cull)
    const float t_ground = best.t;
    const unsigned int cull_ok = (unsigned int)__builtin_amdgcn_readfirstlane(W.hdr[6]);   // leaves whose box was verified to contain their object (csrc/cullflags.hip)
    const int n_eval = __builtin_amdgcn_readfirstlane(W.hdr[0]);
    if (walker) for (int e = 0; e < n_eval; e++) {           // the slab tests that can matter, bounds broadcast from LDS
      float4 a = W.eval[2 * e], b = W.eval[2 * e + 1];
      // a node whose parent no ray of this wave passed is popped by none of them: skipped for the whole wave (pre-order: the parent's
      // bit is final by now).  Sparse scenes (C5: 4.6 of 31 nodes popped per ray) keep the cost of the stack walk, dense ones lose nothing.
      const unsigned int pbit = (unsigned int)as_int(a.w);
      if (pbit != 0u && wballot((H & pbit) != 0u) == 0) continue;
      float t_min = -kFLOAT_MAX, t_max = kFLOAT_MAX;         // tlas_slab without the empty-node test (empty nodes are not in the table)
      float t1 = (a.x - o.x) * rcp.x, t2 = (b.x - o.x) * rcp.x;
      t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
      t1 = (a.y - o.y) * rcp.y; t2 = (b.y - o.y) * rcp.y;
      t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
      t1 = (a.z - o.z) * rcp.z; t2 = (b.z - o.z) * rcp.z;
      t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
      H |= t_max >= t_min ? (unsigned int)as_int(b.w) : 0u;
      if (cull_ok & (unsigned int)__builtin_amdgcn_readfirstlane(as_int(b.w)))      // (wave-uniform: the entry is broadcast from LDS)
        Cm |= tlas_cull(t_min, t_max, t_ground) ? (unsigned int)as_int(b.w) : 0u;
    }
    const unsigned int imask = (unsigned int)W.hdr[2];
    const int levels = __builtin_amdgcn_readfirstlane(W.hdr[1]);
    unsigned int Pm = 1u;                                    // popped: the root ...
    for (int dpt = 0; dpt + 1 < levels && dpt < 4; dpt++) {  // ... and the children of popped, hit, interior nodes, level by level
      unsigned int X = Pm & H & imask & (unsigned int)W.hdr[8 + dpt];
      Pm |= (X << 1) | (X << W.hdr[12 + dpt]);
    }
    if (COUNT && walker) lc.tlas_nodes += (unsigned int)__popc(Pm & (unsigned int)W.hdr[3]);     // BVHNode fetches of the reference's walk (bi < count)
    unsigned int src = Pm & H & (unsigned int)W.hdr[4];      // popped and hit leaves: the first one sets `tests` (RS:315), for good
    unsigned int Tn = 0;
    if (src) Tn = Pm & (unsigned int)W.hdr[5] & ~((1u << __builtin_ctz(src)) - 1u);
    if (walker) T = Tn & ~Cm;
  }
  URT_FS(if (walk_now && n_fresh > 0) { fs[0] += wall_clock64() - fs_t0; fs[3]++; fs[6] += (unsigned long long)n_fresh; })
  bool need = false;
  bool has = mine && T != 0;
  for (;;) {
    // (1) every lane works off the single-leaf MeshObjects at the head of its mask, until every lane stands at a big one (or is done)
    int32_t root = kEmptyMeshRoot; int sfirst = -1;
    URT_FS(unsigned long long fs_t1 = wall_clock64();)
    for (;;) {
      if (has) { int p = __builtin_ctz(T); root = W.pos_tab[2 * p]; sfirst = W.pos_tab[2 * p + 1]; }
      bool small = has && root < 0;
      if (wballot(small) == 0) break;
      URT_FS(fs[4]++;)
      if (small) {
        int bi_local = -1;
        if (L.small_tris) test_leaf<COUNT>(S, root, o, d, best, bi_local, lc, L.small_tris, sfirst);
        else test_leaf<COUNT>(S, root, o, d, best, bi_local, lc);
        T &= T - 1u; has = T != 0;
      }
    }
    URT_FS(fs[1] += wall_clock64() - fs_t1; fs_t1 = wall_clock64();)
    // (2) ONE walk of the LDS-resident BVH top for all the lanes that now stand at a big MeshObject
    if (wballot(has) == 0) break;
    URT_FS(fs[5]++;)
    if (has) {
      sp = SP0;
      if (root < P.top_nodes) {
        BlasRay R = blas_ray(o, d);
        if (SP0 == 1) root = blas_walk_top_ptr<COUNT, CONES>(top, P.top_nodes, root, R, best.t, bl, sp, lc, CONES ? cone_ray_word(d) : 0);
        else do root = blas_node_step_top<COUNT>(top, root, R, best.t, bl, sp, lc); while (root >= 0 && root < P.top_nodes);
      }
      T &= T - 1u;
      if (root == kBlasDone) has = T != 0;                   // nothing of this mesh is near the ray
      else { cur = root; need = true; has = false; }         // on to the BLAS phase; the mask continues at RESUME
    }
    URT_FS(fs[2] += wall_clock64() - fs_t1;)
  }
  cs = (int)T;
  if (mine && !need && S.n_spheres > 0) {                    // IntersectSphereBVH RS:329-361
    v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
    int c2 = 1; tl[0] = 0; bool seen2 = false;
    while (c2 > 0) {
      c2--;
      int bi = tl[c2 * 64];
      bool hit = false; int index = -1;
      if (bi < S.n_sphere_tlas) {
        if (COUNT) lc.tlas_nodes++;
        float4 a, b;
        if (L.sphere_tlas) { a = L.sphere_tlas[2 * bi]; b = L.sphere_tlas[2 * bi + 1]; } else { a = S.sphere_tlas[2 * bi]; b = S.sphere_tlas[2 * bi + 1]; }
        index = as_int(a.w);
        hit = tlas_slab(a, b, o, rcp);
      }
      if (hit) {
        if (index < 0) { tl[c2 * 64] = bi * 2 + 1; c2++; tl[c2 * 64] = bi * 2 + 2; c2++; }
        else seen2 = true;
      }
      if (seen2 && index >= 0 && index < S.n_spheres) intersect_sphere<COUNT>(S, index, o, d, best, lc, L.sphere_pr);
    }
  }
  return put_off ? 2 : need ? 1 : 0;
}

enum : int { ST_DEAD = 0, ST_FRONT = 1, ST_RESUME = 2, ST_BLAS = 3, ST_SHADE = 4, ST_SKY = 5 };

// The work of a batched launch, in tiles: the frames' tile sequences one after the other, or — frames interleaved in groups of
// P.frame_group (wave_fetch_pixels) — whole groups of whole runs of P.xcd_run tiles.
__device__ __forceinline__ unsigned int launch_tiles(const FrameParams& P, unsigned int& tiles_per_frame) {
  tiles_per_frame = (unsigned int)(P.tiles_x * P.n_strips);
  return P.frame_group <= 1 ? tiles_per_frame * (unsigned int)P.n_frames
                            : (((unsigned int)P.n_frames + (unsigned int)P.frame_group - 1u) / (unsigned int)P.frame_group) * (unsigned int)P.frame_group *
                              ((tiles_per_frame + (unsigned int)P.xcd_run - 1u) / (unsigned int)P.xcd_run) * (unsigned int)P.xcd_run;
}

}  // namespace
