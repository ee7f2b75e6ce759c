// shade_device.h — Shade (RS:386-428) and what it calls, shared by the frame kernels (kernels.hip) and the radiance queries
// (radiance.hip): SampleHemisphere, the surface-hit half, the sky-miss half and their union.  The functions are the frame kernels' own,
// moved here unchanged.  Internal to the library; included by .hip translation units only, after trace_device.h and sky_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"
#include "trace_device.h"
#include "sky_device.h"

using namespace urt;
using namespace urtd;

namespace {

// ---------------------------------------------------------------------------------------------------
// Shade — RS:386-428 (+ SampleHemisphere RS:103-111, GetTangentSpace RS:89-100, sky lookup A.11)
// ---------------------------------------------------------------------------------------------------
// inv_alpha1 = 1 / (alpha + 1) (RS:104), precomputed per material on the host (scene_prep.cpp pack_material); 0.5 for the diffuse lobe
__device__ __forceinline__ v3 sample_hemisphere(v3 normal, float inv_alpha1, float& seed, float px, float py) {
  float cosTheta = f_pow(rand_next(seed, px, py), inv_alpha1);
  float sinTheta = f_sqrt(1.0f - cosTheta * cosTheta);
  float phi = (2.0f * kPI) * rand_next(seed, px, py);
  float sp, cp; f_sincos(phi, sp, cp);
  v3 ts = mk3(cp * sinTheta, sp * sinTheta, cosTheta);
  v3 helper = mk3(1, 0, 0);
  if (f_abs(normal.x) > 0.99f) helper = mk3(0, 0, 1);
  v3 tangent = normalize(cross(normal, helper));
  v3 binormal = normalize(cross(normal, tangent));
  return mk3(f_fma(ts.z, normal.x, f_fma(ts.y, binormal.x, ts.x * tangent.x)),
             f_fma(ts.z, normal.y, f_fma(ts.y, binormal.y, ts.x * tangent.y)),
             f_fma(ts.z, normal.z, f_fma(ts.y, binormal.z, ts.x * tangent.z)));
}

// One bounce's shading: result += energy_before * Shade(ray, hit) (A.3); returns any(energy) (RS:457).
// The two halves of Shade (surface hit RS:388-419, sky miss RS:420-427) are separate functions: the phase-scheduled kernel
// runs them as separate phases (lanes of one wave that ended on the sky do not sit through the surface code and vice versa).
template <bool COUNT>
__device__ __forceinline__ bool shade_surface(const DevScene& S, const HitRec& h, v3& o, v3& d, v3& energy, v3& result,
                                              float& seed, float px, float py, LocalCounters& lc) {
  v3 e0 = energy;
  v3 s;
  {
    v3 pos = madd(h.t, d, o);
    v3 n;
    int mat;                                   // one material table: spheres, then mesh objects, then the ground plane
    if (h.kind() == 1) {                       // RS:164-170
      if (COUNT) lc.hit_ground++;
      n = mk3(0, 1, 0);
      mat = S.n_spheres + S.n_meshes;
    } else if (h.kind() == 2) {                // RS:192-194
      if (COUNT) lc.hit_sphere++;
      n = normalize(pos - xyz(S.sphere_pr[h.id()]));
      mat = h.id();
    } else {                                   // RS:259-264
      if (COUNT) lc.hit_tri++;
      const float4* tn = S.tri_norms + 3 * (size_t)h.id();
      v3 n0 = xyz(tn[0]), n1 = xyz(tn[1]), n2 = xyz(tn[2]);
      float w = 1.0f - h.u - h.v;
      n = normalize((n0 * w) + (n1 * h.u) + (n2 * h.v));
      mat = S.n_spheres + as_int(S.tri_verts[3 * (size_t)h.id() + 1].w);
    }
    // what RS:390-395, 401, 404-405, 411 derive from the material alone comes precomputed (scene_prep.cpp pack_material)
    const float4* m = S.materials + 4 * (size_t)mat;
    float4 m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
    float specChance = m0.w, bothChances = m1.w, diffChance = m2.w;
    float roulette = rand_next(seed, px, py);
    // RS:399-418.  The specular and the diffuse branch both end in SampleHemisphere: lanes of one wave take either, so the
    // branch-specific inputs (lobe axis, 1/(alpha+1)) are selected first and the long common part runs ONCE for both kinds
    // of lane.  Per lane the operations and their order are those of the two-branch form.
    bool is_spec = roulette < specChance;
    bool is_diff = !is_spec && diffChance > 0 && roulette < bothChances;
    if (is_spec || is_diff) {
      float inv_alpha1 = 0.5f;                 // diffuse: alpha = 1 (RS:410)
      v3 axis = n;
      if (is_spec) { inv_alpha1 = m3.y; axis = reflect(d, n); }
      o = madd(0.001f, n, pos);
      d = sample_hemisphere(axis, inv_alpha1, seed, px, py);
      if (is_spec) {
        float sd = f_saturate(dot(n, d) * m3.z);
        energy = energy * (xyz(m1) * sd);
      } else {
        energy = energy * xyz(m0);
      }
    } else {
      energy = mk3(0, 0, 0);
    }
    s = xyz(m2);
  }
  result = result + e0 * s;
  return any_nonzero(energy);
}

template <bool COUNT>
__device__ __forceinline__ bool shade_sky(const DevScene& S, v3 d, v3& energy, v3& result, LocalCounters& lc) {
  v3 e0 = energy;
  if (COUNT) lc.hit_sky++;
  energy = mk3(0, 0, 0);
  v3 s = sky_radiance(S, d);                   // RS:424-426 (sky_device.h)
  result = result + e0 * s;
  return any_nonzero(energy);                  // false: the path ends here (RS:421,457)
}

template <bool COUNT>
__device__ __forceinline__ bool shade(const DevScene& S, const HitRec& h, v3& o, v3& d, v3& energy, v3& result,
                                      float& seed, float px, float py, LocalCounters& lc) {
  if (h.t < URT_INF) return shade_surface<COUNT>(S, h, o, d, energy, result, seed, px, py, lc);
  return shade_sky<COUNT>(S, d, energy, result, lc);
}

}  // namespace
