// query_device.h — the fields of a hit record, shared by the ray queries (query.hip k_query) and the feature buffers (aov.hip k_aov).
// Internal to the library; included by .hip translation units only, after trace_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "trace_device.h"

namespace {

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

}  // namespace
