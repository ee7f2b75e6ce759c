// query_device.h — one ray's trace outside a frame and the fields of its hit record, shared by the ray queries (query.hip k_query) and
// the feature buffers (aov.hip k_aov).  The walk is frame_device.h trace() — the same device functions (trace_device.h), the same arithmetic,
// the reference's "tests never reset" object walk (A.5) and the (t, index slot) tie rule — bounded by t_max.  Internal to the library;
// included by .hip translation units only, after trace_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "trace_device.h"

namespace {

// intersect_mesh with an early exit after the first leaf that produced a hit (any-hit form)
__device__ __forceinline__ void intersect_mesh_any(const DevScene& S, int32_t root, v3 o, v3 d, HitRec& best, int* stk, LocalCounters& lc) {
  if (root == kEmptyMeshRoot) return;
  BlasRay R = blas_ray(o, d);
  int best_i = -1;
  int sp = 0;
  int32_t cur = root;
  while (cur != kBlasDone) {
    if (cur >= 0) {
      cur = blas_node_step<false>(S, cur, R, best.t, stk, sp, lc);
    } else {
      test_leaf<false>(S, cur, o, d, best, best_i, lc);
      if (best.kid != 0) return;
      cur = blas_pop(stk, sp);
    }
  }
}

// trace() of frame_device.h bounded by t_max (> 0, not NaN: the caller answers the others with a miss); kind 0 = nothing with t < t_max
template <bool ANY>
__device__ __forceinline__ HitRec query_trace(const DevScene& S, v3 o, v3 d, float t_max, int* tl, int* bl) {
  LocalCounters lc;                                             // never counted: queries leave urt_counters alone
  HitRec best; best.t = t_max; best.kid = 0; best.u = 0; best.v = 0;
  float t_ground = URT_INF;                                     // what trace() hands the object-level cull: the ground hit, t_max aside
  {
    float t = -o.y / d.y;
    if (t > 0 && t < URT_INF) t_ground = t;
    if (t > 0 && t < best.t) { best.t = t; best.kid = 1; }
    if (ANY && best.kid != 0) return best;
  }
  v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
  if (S.n_meshes > 0) {
    int check = 1; tl[0] = 0; bool seen = false;
    while (check > 0) {
      check--;
      int bi = tl[check * 64];
      bool hit = false, culled = false; int index = -1;
      if (bi < S.n_mesh_tlas) {
        float4 a = S.mesh_tlas[2 * bi], b = S.mesh_tlas[2 * bi + 1];
        index = as_int(a.w);
        float t_min, t_max2;
        hit = tlas_slab_t(a, b, o, rcp, t_min, t_max2);
        culled = leaf_culled(b, t_min, t_max2, t_ground);
      }
      if (hit) {
        if (index < 0) { tl[check * 64] = bi * 2 + 1; check++; tl[check * 64] = bi * 2 + 2; check++; }
        else seen = true;
      }
      if (seen && !culled && index >= 0 && index < S.n_meshes) {
        if (ANY) {
          intersect_mesh_any(S, S.mesh_root[index], o, d, best, bl, lc);
          if (best.kid != 0) return best;
        } else {
          intersect_mesh<false>(S, S.mesh_root[index], o, d, best, bl, lc);
        }
      }
    }
  }
  if (S.n_spheres > 0) {
    int check = 1; tl[0] = 0; bool seen = false;
    while (check > 0) {
      check--;
      int bi = tl[check * 64];
      bool hit = false; int index = -1;
      if (bi < S.n_sphere_tlas) {
        float4 a = S.sphere_tlas[2 * bi], b = S.sphere_tlas[2 * bi + 1];
        index = as_int(a.w);
        hit = tlas_slab(a, b, o, rcp);
      }
      if (hit) {
        if (index < 0) { tl[check * 64] = bi * 2 + 1; check++; tl[check * 64] = bi * 2 + 2; check++; }
        else seen = true;
      }
      if (seen && index >= 0 && index < S.n_spheres) {
        intersect_sphere<false>(S, index, o, d, best, lc);
        if (ANY && best.kid != 0) return best;
      }
    }
  }
  return best;
}

// The urt_RayHit record of a trace as three float4: r0 = distance, position.xyz | r1 = normal.xyz, kind (int bits) | r2 = object, primitive
// (int bits), u, v.  object = sphere or MeshObject index, primitive = index slot i of RS:243 (-1 where none).  A miss: (+inf, 0, 0, 0),
// (0, 0, 0, 0), (-1, -1, 0, 0).
struct HitRecord { float4 r0, r1, r2; };
__device__ __forceinline__ HitRecord hit_record(const DevScene& S, const HitRec& h, v3 o, v3 d) {
  float4 r0 = make_float4(URT_INF, 0, 0, 0), r1 = make_float4(0, 0, 0, 0), r2 = make_float4(as_float(-1), as_float(-1), 0, 0);
  if (h.kind() != 0) {
    // position and normal: the expressions of shade_device.h shade_surface (RS:164-170, 192-194, 259-264)
    v3 pos = madd(h.t, d, o);
    v3 nrm;
    int object = -1, primitive = -1;
    float u = 0, v = 0;
    if (h.kind() == 1) {
      nrm = mk3(0, 1, 0);
    } else if (h.kind() == 2) {
      nrm = normalize(pos - xyz(S.sphere_pr[h.id()]));
      object = h.id();
    } else {
      const float4* tn = S.tri_norms + 3 * (size_t)h.id();
      v3 n0 = xyz(tn[0]), n1 = xyz(tn[1]), n2 = xyz(tn[2]);
      float w = 1.0f - h.u - h.v;
      nrm = normalize((n0 * w) + (n1 * h.u) + (n2 * h.v));
      primitive = as_int(S.tri_verts[3 * (size_t)h.id()].w);      // index slot i of RS:243
      object = as_int(S.tri_verts[3 * (size_t)h.id() + 1].w);     // MeshObject
      u = h.u; v = h.v;
    }
    r0 = make_float4(h.t, pos.x, pos.y, pos.z);
    r1 = make_float4(nrm.x, nrm.y, nrm.z, as_float(h.kind()));
    r2 = make_float4(as_float(object), as_float(primitive), u, v);
  }
  return {r0, r1, r2};
}

typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_nt(float4* p, float4 v) {   // streaming store: the results are not read again by the kernel
  f4v w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, (f4v*)p);
}

}  // namespace
