// cones.hip — normal cones of the triangle-BVH children (option "blas_cones"): one dword per child in the two spare dwords of the traversal's
// (centre, half extent) nodes, cnodes[4n + 3].z for child 0 and .w for child 1.  The scheduled trace kernel skips a child whose triangles
// the ray can only see from behind (trace_device.h cone_skips): Moller-Trumbore with back-face culling (RS:199-234) rejects every one of
// them, so nothing the walk would have found there can change the closest hit — the skip is exact, pixels do not change.
//
// The word: four signed bytes (ax, ay, az, T).  The ray's word: r = (round(127 d.x), round(127 d.y), round(127 d.z), -127).  The child is
// skipped iff  ax rx + ay ry + az rz - 127 T > 0  (one v_dot4c and a compare); word 0 never skips.
//
// The obligation on T.  If the test skips for a direction d with | |d| - 1 | <= 2^-10, then every triangle (e1, e2) below the child has, in
// real arithmetic, d . (e1 x e2) >= 2^-16 |e1| |e2|.  The normative det is -d . (e1 x e2) up to a few ulps of |e1| |e2| |d| (about 4e-7,
// forty times less), so the computed det is negative, hence < kEPSILON.
//
// The margin.  A = (ax, ay, az), a~ = A / |A| — the cone is measured about the QUANTIZED axis, so the axis costs no error —, u = d / |d|,
// n_i the unit normals, phi the largest angle between a~ and an n_i, sin theta_i = |e1 x e2| / (|e1| |e2|) and
// mu = max_i 2^-16 / (sin theta_i (1 - 2^-10)).  d . (e1 x e2) >= 2^-16 |e1| |e2| follows from u . n_i >= mu; with u . a~ = cos alpha it
// is u . n_i >= cos(alpha + phi), so cos alpha >= sin(phi + kappa), sin kappa = mu, is enough — valid only while phi + kappa < pi / 2,
// i.e. cos phi > mu — and sin(phi + kappa) <= sin phi + mu =: s.  The ray bytes are R = 127 d + e with |e_k| <= 0.5001 (rounding to
// nearest, and the float product), |e| <= 0.8663, so A . R = 127 |A| |d| (a~ . u) + A . e and a skip (A . R > 127 T) gives
//     a~ . u > (127 T - 0.8663 |A|) / (127 |A| (1 + 2^-10))  >=  s     as soon as     T >= |A| (s (1 + 2^-10) + 0.8663 / 127).
// T is that bound rounded up to an integer; a bound above 127 does not fit the byte: word 0.  With |A| about 127 the two quantisations cost
// (0.87 + the rounding up) / 127, about 0.014 in cosine.
// The arithmetic here is float32 and not normative; every rounding is padded outwards: mu by 10 % (the computed normal of a sliver is
// off by up to 2^-22 / sin theta, a sixtieth of mu), the sine of phi — taken as max |n_i x a~|, no cancellation — and cos phi by 4e-6,
// the bound on T by 1e-5.  A child gets word 0 when a triangle below it has no area, is too thin for the margin (mu >= cos phi), when
// the windings are mixed or the spread reaches a right angle (cos phi <= mu), on any NaN or infinity, and when its triangles are not
// contiguous in leaf order.  tests/cones_ref.py restates the decode and the test; tests/test_cones_ref.py and tests/test_gpu_cones.py
// check the obligation in float64, the latter on the words and triangle records read back from the device.
//
// A child's triangles are a contiguous range of leaf-order slots (every builder emits a subtree's leaves next to each other); the ranges
// are found once per scene by relaxation from the leaves, one sweep per tree level (k_range_step), and survive refits (the topology
// does); one wave per child then reduces its range twice: normals' sum -> axis, then spread and thinnest triangle about that axis.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "cones.h"

using namespace urt;

namespace {

constexpr int kUnknown = -1, kScattered = -2;      // range.first of a child not resolved yet / whose triangles are not contiguous

// int4 per node: first0, count0, first1, count1
__global__ __launch_bounds__(256) void k_range_init(const float4* __restrict__ nodes, int n_nodes, int4* __restrict__ rng) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  float4 q3 = nodes[4 * (size_t)n + 3];
  const int32_t c[2] = {__builtin_bit_cast(int, q3.x), __builtin_bit_cast(int, q3.y)};
  int r[4];
  for (int j = 0; j < 2; j++) {
    uint32_t code = ~(uint32_t)c[j];
    r[2 * j] = c[j] < 0 ? (int)(code >> 3) : kUnknown;
    r[2 * j + 1] = c[j] < 0 ? (int)(code & 7u) + 1 : 0;
  }
  rng[n] = make_int4(r[0], r[1], r[2], r[3]);
}

__global__ __launch_bounds__(256) void k_range_step(const float4* __restrict__ nodes, int n_nodes, const int4* __restrict__ src, int4* __restrict__ dst) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  int4 me = src[n];
  int r[4] = {me.x, me.y, me.z, me.w};
  if (r[0] == kUnknown || r[2] == kUnknown) {
    float4 q3 = nodes[4 * (size_t)n + 3];
    const int32_t c[2] = {__builtin_bit_cast(int, q3.x), __builtin_bit_cast(int, q3.y)};
    for (int j = 0; j < 2; j++) {
      if (r[2 * j] != kUnknown) continue;
      if (c[j] < 0 || c[j] >= n_nodes) { r[2 * j] = kScattered; continue; }        // (a leaf is resolved by k_range_init; an index outside the pool: no cone)
      int4 k = src[c[j]];
      if (k.x == kUnknown || k.z == kUnknown) continue;
      if (k.x == kScattered || k.z == kScattered) { r[2 * j] = kScattered; continue; }
      int lo = min(k.x, k.z), hi = max(k.x + k.y, k.z + k.w);
      r[2 * j] = hi - lo == k.y + k.w ? lo : kScattered;
      r[2 * j + 1] = k.y + k.w;
    }
  }
  dst[n] = make_int4(r[0], r[1], r[2], r[3]);
}

__device__ __forceinline__ float wave_sum(float v) { for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64)); return v; }
__device__ __forceinline__ float wave_min(float v) { for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s, 64)); return v; }

// unit normal of leaf-order triangle k; thin = 2^-16 |e1| |e2| / |e1 x e2|; false: no area, or not finite
__device__ __forceinline__ bool tri_normal(const float4* __restrict__ tri_verts, int k, float n[3], float& thin) {
  float4 a = tri_verts[3 * (size_t)k + 1], b = tri_verts[3 * (size_t)k + 2];
  float gx = a.y * b.z - a.z * b.y, gy = a.z * b.x - a.x * b.z, gz = a.x * b.y - a.y * b.x;
  float g2 = gx * gx + gy * gy + gz * gz;
  float l2 = (a.x * a.x + a.y * a.y + a.z * a.z) * (b.x * b.x + b.y * b.y + b.z * b.z);
  // (a triangle whose squares under- or overflow float32 gets no cone: 1e-30 < g2, l2 < 1e30)
  if (!(g2 > 1e-30f && g2 < 1e30f && l2 > 1e-30f && l2 < 1e30f)) { n[0] = n[1] = n[2] = 0.0f; thin = 0.0f; return false; }
  float inv = 1.0f / sqrtf(g2);
  n[0] = gx * inv; n[1] = gy * inv; n[2] = gz * inv;
  thin = 1.52587890625e-5f * sqrtf(l2) * inv;
  return true;
}

// one wave per child: child id = 2 n + j
__global__ __launch_bounds__(256) void k_cones(const int4* __restrict__ rng, int n_nodes, const float4* __restrict__ tri_verts, int n_tris, float4* __restrict__ cnodes) {
  const int lane = threadIdx.x & 63;
  const long id = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);       // wave-uniform
  if (id >= 2 * (long)n_nodes) return;
  const int n = (int)(id >> 1), j = (int)(id & 1);
  int4 r = rng[n];
  const int first = j ? r.z : r.x, count = j ? r.w : r.y;
  int word = 0;
  // (the whole wave takes the same branches: first and count are wave-uniform)
  if (first >= 0 && count > 0 && first <= n_tris - count) {
    float sx = 0, sy = 0, sz = 0, thin = 0, bad = 0;
    for (int k = lane; k < count; k += 64) {
      float nn[3], t;
      if (!tri_normal(tri_verts, first + k, nn, t)) bad = 1.0f;
      sx += nn[0]; sy += nn[1]; sz += nn[2]; thin = fmaxf(thin, t);
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); thin = wave_max(thin); bad = wave_max(bad);
    float sl = sqrtf(sx * sx + sy * sy + sz * sz);
    if (bad == 0.0f && sl > 1e-3f && sl < 1e30f) {
      // the quantized axis, and the cone about IT
      float ax = rintf(127.0f * (sx / sl)), ay = rintf(127.0f * (sy / sl)), az = rintf(127.0f * (sz / sl));
      float an = sqrtf(ax * ax + ay * ay + az * az);
      float ux = ax / an, uy = ay / an, uz = az / an;
      float cmin = 2.0f, smax = 0.0f;
      for (int k = lane; k < count; k += 64) {
        float nn[3], t;
        tri_normal(tri_verts, first + k, nn, t);
        cmin = fminf(cmin, nn[0] * ux + nn[1] * uy + nn[2] * uz);
        float cx = nn[1] * uz - nn[2] * uy, cy = nn[2] * ux - nn[0] * uz, cz = nn[0] * uy - nn[1] * ux;
        smax = fmaxf(smax, cx * cx + cy * cy + cz * cz);
      }
      cmin = wave_min(cmin) - 4e-6f; smax = sqrtf(wave_max(smax)) + 4e-6f;
      float mu = thin * (1.1f / (1.0f - 9.765625e-4f));
      if (cmin > mu && mu < 1.0f) {                            // phi + kappa < pi / 2 (a NaN fails the compare)
        float s = smax + mu;
        float tb = an * (s * (1.0f + 9.765625e-4f) + 0.8663f / 127.0f) * 1.00001f;
        float T = ceilf(tb);
        if (T <= 127.0f) word = ((int)ax & 0xff) | (((int)ay & 0xff) << 8) | (((int)az & 0xff) << 16) | (((int)T & 0xff) << 24);
      }
    }
  }
  if (lane == 0) ((int*)cnodes)[16 * (size_t)n + 14 + j] = word;
}

}  // namespace

namespace urtd {

hipError_t cone_ranges(const float4* nodes, int n_nodes, int max_depth, int4* rng_a, int4* rng_b, const int4** out, hipStream_t st) {
  *out = rng_a;
  if (n_nodes <= 0) return hipSuccess;
  const dim3 grid((n_nodes + 255) / 256), block(256);
  hipLaunchKernelGGL(k_range_init, grid, block, 0, st, nodes, n_nodes, rng_a);
  int4 *src = rng_a, *dst = rng_b;
  // a child at height h above the leaves is resolved after h sweeps; a child left unknown by a wrong depth simply gets no cone
  for (int s = 0; s < max_depth; s++) {
    hipLaunchKernelGGL(k_range_step, grid, block, 0, st, nodes, n_nodes, (const int4*)src, dst);
    int4* t = src; src = dst; dst = t;
  }
  *out = src;
  return hipGetLastError();
}

hipError_t cone_words(const int4* rng, int n_nodes, const float4* tri_verts, int n_tris, float4* cnodes, hipStream_t st) {
  if (n_nodes <= 0) return hipSuccess;
  const long waves = 2 * (long)n_nodes;
  hipLaunchKernelGGL(k_cones, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rng, n_nodes, tri_verts, n_tris, cnodes);
  return hipGetLastError();
}

}  // namespace urtd
