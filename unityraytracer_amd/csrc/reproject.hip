// reproject.hip — temporal reprojection of an accumulated image across a camera move (urt_reproject) and the AdditionShader blend with a
// per-pixel sample count (urt_blit_add_history).  include/urt.h states the arithmetic; the library is built with -ffp-contract=off, so
// every expression below is evaluated with one rounding per operation, as written there.
//
// k_reproject: one pixel per lane, wave64.  A wave covers one 8 x 8 pixel tile and a 256-thread workgroup a 16 x 16 block, as k_aov /
// k_denoise_*.  A pixel loads its three current feature texels, projects its hit point (or, for a sky pixel, its pixel-centre direction)
// into the previous view and gathers the 2 x 2 bilinear footprint around it from the previous history and feature buffers: for small
// motions the taps of a wave are the wave's own 8 x 8 block shifted, so they coalesce as the current loads do.  No LDS.
// k_reproject<true> (urt_reproject_objects) is the same kernel instantiated with MOTION: a triangle or sphere pixel also loads its
// object's 48-byte "current world -> previous world" entry (three dwordx4 loads; the object id is uniform over most waves, so the entry
// comes from one or two cache lines) and projects the point where it WAS.  Ground, sky and scenes without tables pay one uniform branch;
// k_reproject<false> keeps its argument struct and takes none of the new branches.
// k_reproject<true, ParamsDeform> (urt_reproject_deformed) is a third instantiation: a triangle pixel of a MeshObject flagged as deformed
// finds the point it shows where the previous vertex positions of its triangle put it: three dword index loads, three 12-byte vertex
// gathers and the object's previous matrix as four dwordx4 loads (the object id is uniform over most waves; lanes of one triangle ask
// for the same addresses, which one cache line serves).  Every index is checked against its buffer before it is used.  The two other
// instantiations keep their argument structs and their code.
// k_blit_add_history / k_blit_add_history_multi: grid-stride over the pixels as k_blit_add / k_blit_add_multi; the fused form reads the
// count and dst once, blends n frames and writes both (and the present) once: 16 n + 64 bytes per pixel with a present.
#include <hip/hip_runtime.h>

#include "../../include/urt_math.h"
#include "reproject.h"

namespace {

struct Params {
  urtd::ReprojectImages I;
  urtd::ReprojectSettings P;
};

struct ParamsObjects : Params {
  urtd::ReprojectMotion T;
};

struct ParamsDeform : ParamsObjects {
  urtd::ReprojectDeform D;
};

template <class PARAMS> struct is_deform { static constexpr bool value = false; };
template <> struct is_deform<ParamsDeform> { static constexpr bool value = true; };

struct Vec3 { float x, y, z; };                                  // an element of a stride-12 buffer

__device__ __forceinline__ bool finite3(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
__device__ __forceinline__ bool finite4(float4 v) { return finite3(v) && isfinite(v.w); }

// the twelve floats of an entry are bit for bit (1,0,0, 0,1,0, 0,0,1, 0,0,0)
__device__ __forceinline__ bool identity_entry(float4 a, float4 b, float4 c) {
  const int one = 0x3f800000;
  return ((__float_as_int(a.x) ^ one) | __float_as_int(a.y) | __float_as_int(a.z) | __float_as_int(a.w) | (__float_as_int(b.x) ^ one) |
          __float_as_int(b.y) | __float_as_int(b.z) | __float_as_int(b.w) | (__float_as_int(c.x) ^ one) | __float_as_int(c.y) |
          __float_as_int(c.z) | __float_as_int(c.w)) == 0;
}

// urt_reproject (MOTION false, PARAMS = Params) and urt_reproject_objects (MOTION true, PARAMS = ParamsObjects).  A pixel that is not
// moved takes exactly the operations of the instantiation without MOTION.  urt_reproject_deformed (MOTION true, PARAMS = ParamsDeform):
// a pixel that is not deformed takes exactly the operations of urt_reproject_objects.
template <bool MOTION, class PARAMS>
__global__ __launch_bounds__(256) void k_reproject(const PARAMS A) {
  constexpr bool DEFORM = is_deform<PARAMS>::value;
  const urtd::ReprojectImages& I = A.I;
  const urtd::ReprojectSettings& P = A.P;
  const urtd::ReprojectMotion* T = nullptr;
  if constexpr (MOTION) T = &A.T;
  const int W = I.width, H = I.height;
  // workgroup = 16 x 16 pixels, wave = the 8 x 8 tile (wave & 1, wave >> 1) of it, lane = (lane & 7, lane >> 3) of the tile
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= W || y >= H) return;                                  // partial tiles at the right and top edges
  const size_t pix = (size_t)y * (size_t)W + (size_t)x;

  const float4 h = I.hit[pix], nr = I.normal[pix];
  const float k = nr.w, z = h.w;
  const bool sky = k == 0.0f;
  const bool surface_in = !sky && isfinite(z) && z > 0.0f && finite3(h) && finite3(nr);
  const float* M = P.m;

  // the point and the normal the previous frame knew this surface by: the pixel's own unless its object has moved
  float4 hp = h, np = nr;
  float L = 1.0f;
  bool moved = false, dead = false;
  bool deformed = false;
  if constexpr (DEFORM) {
    const urtd::ReprojectDeform& D = A.D;
    if (surface_in && k == 3.0f && D.flags) {                    // (uniform; null flags = no deform, reproject.h: the host then launches <true, ParamsObjects>)
      const float4 idp = I.id[pix];
      const int o = __float_as_int(idp.x);
      if (o < 0 || o >= D.n_objects) {
        dead = true;                                             // no such MeshObject: no history
      } else if (D.flags[o] != 0) {
        deformed = true;
        dead = true;                                             // until the previous triangle is found and sound
        const int i = __float_as_int(idp.y);
        const float u = idp.z, v = idp.w;
        if (i >= 0 && i <= D.n_indices - 3) {
          const int j0 = D.indices[i], j1 = D.indices[i + 1], j2 = D.indices[i + 2];
          const int nv = D.n_vertices;
          if (j0 >= 0 && j0 < nv && j1 >= 0 && j1 < nv && j2 >= 0 && j2 < nv) {
            const Vec3* vp = (const Vec3*)D.vertices;
            const Vec3 a0 = vp[j0], a1 = vp[j1], a2 = vp[j2];
            const float4* mp = D.objects + 7 * (size_t)o;        // a MeshObject: 112 bytes, localToWorldMatrix first
            const float4 c0 = mp[0], c1 = mp[1], c2 = mp[2], c3 = mp[3];   // its columns
            const float v0x = ((c0.x * a0.x + c1.x * a0.y) + c2.x * a0.z) + c3.x;
            const float v0y = ((c0.y * a0.x + c1.y * a0.y) + c2.y * a0.z) + c3.y;
            const float v0z = ((c0.z * a0.x + c1.z * a0.y) + c2.z * a0.z) + c3.z;
            const float v1x = ((c0.x * a1.x + c1.x * a1.y) + c2.x * a1.z) + c3.x;
            const float v1y = ((c0.y * a1.x + c1.y * a1.y) + c2.y * a1.z) + c3.y;
            const float v1z = ((c0.z * a1.x + c1.z * a1.y) + c2.z * a1.z) + c3.z;
            const float v2x = ((c0.x * a2.x + c1.x * a2.y) + c2.x * a2.z) + c3.x;
            const float v2y = ((c0.y * a2.x + c1.y * a2.y) + c2.y * a2.z) + c3.y;
            const float v2z = ((c0.z * a2.x + c1.z * a2.y) + c2.z * a2.z) + c3.z;
            const float w = (1.0f - u) - v;
            hp.x = (v0x * w + v1x * u) + v2x * v;
            hp.y = (v0y * w + v1y * u) + v2y * v;
            hp.z = (v0z * w + v1z * u) + v2z * v;
            const float e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
            const float e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
            np.x = e1y * e2z - e1z * e2y;
            np.y = e1z * e2x - e1x * e2z;
            np.z = e1x * e2y - e1y * e2x;
            L = urt::f_sqrt((np.x * np.x + np.y * np.y) + np.z * np.z);
            if (finite3(hp) && L > 0.0f && isfinite(L)) { dead = false; moved = true; }
          }
        }
      }
    }
  }
  if (MOTION && surface_in && (k == 2.0f || k == 3.0f) && !(DEFORM && (deformed || dead))) {
    const float4* tab = k == 3.0f ? T->mesh : T->sphere;
    if (tab) {                                                   // uniform: a scene without tables stops here
      const int o = __float_as_int(I.id[pix].x);
      if (o < 0 || o >= (k == 3.0f ? T->n_mesh : T->n_sphere)) {
        dead = true;                                             // no such entry: no history
      } else {
        const float4 a = tab[3 * (size_t)o], b = tab[3 * (size_t)o + 1], c = tab[3 * (size_t)o + 2];   // a[0..3], a[4..7], a[8..11]
        if (!identity_entry(a, b, c)) {
          moved = true;
          hp.x = ((a.x * h.x + a.w * h.y) + b.z * h.z) + c.y;
          hp.y = ((a.y * h.x + b.x * h.y) + b.w * h.z) + c.z;
          hp.z = ((a.z * h.x + b.y * h.y) + c.x * h.z) + c.w;
          np.x = (a.x * nr.x + a.w * nr.y) + b.z * nr.z;
          np.y = (a.y * nr.x + b.x * nr.y) + b.w * nr.z;
          np.z = (a.z * nr.x + b.y * nr.y) + c.x * nr.z;
          L = urt::f_sqrt((np.x * np.x + np.y * np.y) + np.z * np.z);
          if (!(finite3(hp) && L > 0.0f && isfinite(L))) dead = true;
        }
      }
    }
  }
  const bool surface = MOTION ? surface_in && !dead : surface_in;

  // 2. the point (w = 1) or the direction (w = 0) in the previous camera's clip space
  float cx = 0.0f, cy = 0.0f, cw = 0.0f;
  if (surface) {
    cx = ((M[0] * hp.x + M[4] * hp.y) + M[8] * hp.z) + M[12];
    cy = ((M[1] * hp.x + M[5] * hp.y) + M[9] * hp.z) + M[13];
    cw = ((M[3] * hp.x + M[7] * hp.y) + M[11] * hp.z) + M[15];
  } else if (sky) {
    const float* C = P.c2w;
    const float* Iv = P.invp;
    const float u = ((float)x + 0.5f) / (float)W * 2.0f - 1.0f;
    const float v = ((float)y + 0.5f) / (float)H * 2.0f - 1.0f;
    const float e0 = (Iv[0] * u + Iv[4] * v) + Iv[12];
    const float e1 = (Iv[1] * u + Iv[5] * v) + Iv[13];
    const float e2 = (Iv[2] * u + Iv[6] * v) + Iv[14];
    const float d0 = (C[0] * e0 + C[4] * e1) + C[8] * e2;
    const float d1 = (C[1] * e0 + C[5] * e1) + C[9] * e2;
    const float d2 = (C[2] * e0 + C[6] * e1) + C[10] * e2;
    cx = (M[0] * d0 + M[4] * d1) + M[8] * d2;
    cy = (M[1] * d0 + M[5] * d1) + M[9] * d2;
    cw = (M[3] * d0 + M[7] * d1) + M[11] * d2;
  }
  const float qx = ((cx / cw + 1.0f) * 0.5f) * (float)W - 0.5f;
  const float qy = ((cy / cw + 1.0f) * 0.5f) * (float)H - 0.5f;
  const bool window = (surface || sky) && cw > 0.0f && qx > -1.0f && qx < (float)W && qy > -1.0f && qy < (float)H;

  float S = 0.0f, N = 0.0f;
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (window) {
    // 3. the bilinear footprint
    const float flx = floorf(qx), fly = floorf(qy);
    const float fx = qx - flx, gx = 1.0f - fx, fy = qy - fly, gy = 1.0f - fy;
    const int x0 = (int)flx, y0 = (int)fly;
    const float wt[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    const int o = __float_as_int(I.id[pix].x);
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
      const float w = wt[t];
      if (!(tx >= 0 && tx < W && ty >= 0 && ty < H && w > 0.0f)) continue;
      const size_t q = (size_t)ty * (size_t)W + (size_t)tx;
      const float4 pc = I.prev_count[q], col = I.prev_color[q], m = I.prev_normal[q];
      bool ok = isfinite(pc.x) && pc.x > 0.0f && finite4(col);
      if (sky) {
        ok = ok && m.w == 0.0f;
      } else {
        const float4 Q = I.prev_hit[q];
        const int oq = __float_as_int(I.prev_id[q].x);
        const float nd = (np.x * m.x + np.y * m.y) + np.z * m.z;
        const float pd = fabsf((np.x * (Q.x - hp.x) + np.y * (Q.y - hp.y)) + np.z * (Q.z - hp.z));
        float nt = MOTION && moved ? P.normal_threshold * L : P.normal_threshold;
        if constexpr (DEFORM) { if (deformed) nt = A.D.normal_threshold * L; }
        const float pt = MOTION && moved ? (P.plane_threshold * z) * L : P.plane_threshold * z;
        ok = ok && m.w == k && oq == o && isfinite(Q.w) && Q.w > 0.0f && nd >= nt && pd <= pt;
      }
      if (ok) {                                                  // 4. in tap order
        S = S + w;
        acc.x = acc.x + w * col.x;
        acc.y = acc.y + w * col.y;
        acc.z = acc.z + w * col.z;
        acc.w = acc.w + w * col.w;
        N = N + w * pc.x;
      }
    }
  }
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float n = 0.0f;
  if (S >= 0.01f) {
    c = make_float4(acc.x / S, acc.y / S, acc.z / S, acc.w / S);
    n = N / S;
    if (P.max_history > 0.0f) n = fminf(n, P.max_history);
    if (MOTION && moved && T->moved_max_history > 0.0f) n = fminf(n, T->moved_max_history);
  }
  I.color[pix] = c;
  I.count[pix] = make_float4(n, 0.0f, 0.0f, 0.0f);
  if (I.motion)
    I.motion[pix] = window ? make_float4(qx - (float)x, qy - (float)y, S, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// the sample count a blend uses: s = 0 for a count that is not finite or negative, else the count, capped at max_history - 1
__device__ __forceinline__ float history_samples(float n, float max_history) {
  if (!isfinite(n) || n < 0.0f) return 0.0f;
  return max_history > 0.0f ? fminf(n, max_history - 1.0f) : n;
}

// k_blit_add's operations with s in place of _Sample
__device__ __forceinline__ float4 blend(float4 c, float4 t, float s) {
  const float a = 1.0f / (s + 1.0f);
  const float ia = 1.0f - a;
  c.x = t.x * a + c.x * ia;
  c.y = t.y * a + c.y * ia;
  c.z = t.z * a + c.z * ia;
  c.w = a * a + c.w * ia;
  return c;
}

__global__ __launch_bounds__(256) void k_blit_add_history(const float4* __restrict__ src, float4* __restrict__ dst, float4* __restrict__ count,
                                                          size_t npix, float max_history) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const float s = history_samples(count[i].x, max_history);
    dst[i] = blend(dst[i], src[i], s);
    count[i] = make_float4(s + 1.0f, 0.0f, 0.0f, 0.0f);
  }
}

__global__ __launch_bounds__(256) void k_blit_add_history_multi(const float4* __restrict__ src, size_t frame_stride, int n,
                                                                float4* __restrict__ dst, float4* __restrict__ count,
                                                                float4* __restrict__ present, size_t npix, float max_history) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    float4 c = dst[i];
    float cnt = count[i].x;
    for (int f = 0; f < n; f++) {
      const float s = history_samples(cnt, max_history);
      c = blend(c, src[(size_t)f * frame_stride + i], s);
      cnt = s + 1.0f;                                            // what the count texel of a separate call would hold
    }
    dst[i] = c;
    count[i] = make_float4(cnt, 0.0f, 0.0f, 0.0f);
    if (present) present[i] = c;
  }
}

size_t grid_of(size_t n_pixels, size_t cap) {
  const size_t nb = (n_pixels + 255) / 256;
  return nb > cap ? cap : nb;
}

}  // namespace

namespace urtd {

hipError_t launch_reproject(const ReprojectImages& I, const ReprojectSettings& P, hipStream_t st) {
  if (I.width <= 0 || I.height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((I.width + 15) / 16), (unsigned int)((I.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_reproject<false, Params>), grid, dim3(256), 0, st, Params{I, P});
  return hipGetLastError();
}

hipError_t launch_reproject_objects(const ReprojectImages& I, const ReprojectSettings& P, const ReprojectMotion& T, hipStream_t st) {
  if (I.width <= 0 || I.height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((I.width + 15) / 16), (unsigned int)((I.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  ParamsObjects A{};
  A.I = I; A.P = P; A.T = T;
  hipLaunchKernelGGL((k_reproject<true, ParamsObjects>), grid, dim3(256), 0, st, A);
  return hipGetLastError();
}

hipError_t launch_reproject_deformed(const ReprojectImages& I, const ReprojectSettings& P, const ReprojectMotion& T, const ReprojectDeform& D,
                                     hipStream_t st) {
  if (I.width <= 0 || I.height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((I.width + 15) / 16), (unsigned int)((I.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  ParamsDeform A{};
  A.I = I; A.P = P; A.T = T; A.D = D;
  hipLaunchKernelGGL((k_reproject<true, ParamsDeform>), grid, dim3(256), 0, st, A);
  return hipGetLastError();
}

hipError_t launch_blit_add_history(const float4* src, float4* dst, float4* count, size_t n_pixels, float max_history, hipStream_t st) {
  if (n_pixels == 0) return hipSuccess;
  hipLaunchKernelGGL(k_blit_add_history, dim3((unsigned)grid_of(n_pixels, 2048)), dim3(256), 0, st, src, dst, count, n_pixels, max_history);
  return hipGetLastError();
}

hipError_t launch_blit_add_history_multi(const float4* src, size_t frame_stride, int n, float4* dst, float4* count, float4* present,
                                         size_t n_pixels, float max_history, hipStream_t st) {
  if (n_pixels == 0 || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_blit_add_history_multi, dim3((unsigned)grid_of(n_pixels, 4096)), dim3(256), 0, st, src, frame_stride, n, dst, count,
                     present, n_pixels, max_history);
  return hipGetLastError();
}

}  // namespace urtd
