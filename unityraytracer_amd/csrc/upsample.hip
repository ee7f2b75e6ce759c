// upsample.hip — guide-driven upsampling (urt_upsample): an image traced on a low pixel grid is reconstructed on the full grid by a
// bilinear gather that takes a low-resolution tap only where the feature buffers of both grids show the same surface.  include/urt.h
// states the arithmetic; the library is built with -ffp-contract=off, so every expression below is evaluated with one rounding per
// operation, as written there.
//
// k_upsample: one full-grid pixel per lane, wave64.  A wave covers one 8 x 8 pixel tile and a 256-thread workgroup a 16 x 16 block, as
// k_reproject.  A pixel loads its feature texels (hit, normal; id unless it is sky), finds its place on the low grid and gathers the
// 2 x 2 bilinear footprint around it from the low colour, count and feature images: the stage-1 taps of a tile fall in a block of
// (8 w / W + 1)^2 low texels, a handful of cache lines the wave shares.  No LDS, no atomics.  Sky taps read neither low_hit nor low_id.
// Stage 2 (the 4 x 4 block of equal weights for a pixel whose four taps all failed) is a rare, divergent branch behind stage 1: a pixel
// that has a result pays only the test.  The optional images are wave-uniform null pointers.  Every tap index is checked against the low
// image before it is used.
#include <hip/hip_runtime.h>

#include "upsample.h"

namespace {

struct Params {
  urtd::UpsampleImages I;
  urtd::UpsampleSettings P;
};

__device__ __forceinline__ bool finite3(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
__device__ __forceinline__ bool finite4(float4 v) { return finite3(v) && isfinite(v.w); }

// what a full-grid pixel asks of a tap
struct Pixel {
  float4 h, n;                  // hit, normal
  float k, pt;                  // kind; plane_threshold * z
  int o;                        // object bits (surface pixels)
  bool sky;
};

struct Sums {
  float S, N;
  float4 A;
};

// one tap of either stage: the texel (tx, ty) of the low grid with weight w, added to the sums when it is valid (include/urt.h step 3)
__device__ __forceinline__ void tap(const urtd::UpsampleImages& I, float normal_threshold, const Pixel& p, int tx, int ty, float w, Sums& s) {
  if (!(tx >= 0 && tx < I.low_width && ty >= 0 && ty < I.low_height)) return;
  const size_t q = (size_t)ty * (size_t)I.low_width + (size_t)tx;
  const float4 col = I.low_color[q], m = I.low_normal[q];
  float nq = 1.0f;
  if (I.low_count) nq = I.low_count[q].x;                       // (uniform)
  bool ok = isfinite(nq) && nq > 0.0f && finite4(col);
  if (p.sky) {
    ok = ok && m.w == 0.0f;
  } else {
    const float4 Q = I.low_hit[q];
    const int oq = __float_as_int(I.low_id[q].x);
    const float nd = (p.n.x * m.x + p.n.y * m.y) + p.n.z * m.z;
    const float pd = fabsf((p.n.x * (Q.x - p.h.x) + p.n.y * (Q.y - p.h.y)) + p.n.z * (Q.z - p.h.z));
    ok = ok && m.w == p.k && oq == p.o && isfinite(Q.w) && Q.w > 0.0f && nd >= normal_threshold && pd <= p.pt;
  }
  if (ok) {                                                      // in tap order
    s.S = s.S + w;
    s.A.x = s.A.x + w * col.x;
    s.A.y = s.A.y + w * col.y;
    s.A.z = s.A.z + w * col.z;
    s.A.w = s.A.w + w * col.w;
    s.N = s.N + w * nq;
  }
}

__global__ __launch_bounds__(256) void k_upsample(const Params A) {
  const urtd::UpsampleImages& I = A.I;
  const urtd::UpsampleSettings& P = A.P;
  const int W = I.width, H = I.height;
  // workgroup = 16 x 16 pixels, wave = the 8 x 8 tile (wave & 1, wave >> 1) of it, lane = (lane & 7, lane >> 3) of the tile
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= W || y >= H) return;                                  // partial tiles at the right and top edges
  const size_t pix = (size_t)y * (size_t)W + (size_t)x;

  // 1. class
  Pixel p;
  p.h = I.hit[pix];
  p.n = I.normal[pix];
  p.k = p.n.w;
  const float z = p.h.w;
  p.sky = p.k == 0.0f;
  const bool surface = !p.sky && isfinite(z) && z > 0.0f && finite3(p.h) && finite3(p.n);
  p.pt = P.plane_threshold * z;
  p.o = 0;

  Sums s{0.0f, 0.0f, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
  bool result = false;
  if (surface || p.sky) {
    if (surface) p.o = __float_as_int(I.id[pix].x);
    // 2. the position on the low grid
    const float qx = (((float)x + 0.5f) * (float)I.low_width) / (float)W - 0.5f;
    const float qy = (((float)y + 0.5f) * (float)I.low_height) / (float)H - 0.5f;
    // 3. stage 1: the bilinear footprint
    const float flx = floorf(qx), fly = floorf(qy);
    const float fx = qx - flx, gx = 1.0f - fx, fy = qy - fly, gy = 1.0f - fy;
    const int x0 = (int)flx, y0 = (int)fly;
    const float wt[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (wt[t] > 0.0f) tap(I, P.normal_threshold, p, x0 + (t & 1), y0 + (t >> 1), wt[t], s);
    result = s.S >= 0.01f;
    // 4. stage 2: the 4 x 4 block around the footprint, equal weights
    if (!result && P.wide_fallback) {
      s = Sums{0.0f, 0.0f, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
#pragma unroll 1
      for (int j = 0; j < 4; j++)
#pragma unroll 1
        for (int i = 0; i < 4; i++) tap(I, P.normal_threshold, p, x0 - 1 + i, y0 - 1 + j, 1.0f, s);
      result = s.S >= 1.0f;
    }
  }

  // 5. output
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float n = 0.0f;
  if (result) {
    c = make_float4(s.A.x / s.S, s.A.y / s.S, s.A.z / s.S, s.A.w / s.S);
    n = (s.N / s.S) * P.count_scale;
    if (p.sky && P.sky_from_albedo && I.albedo) {                // the exact sky at full resolution
      const float4 a = I.albedo[pix];
      c.x = a.x; c.y = a.y; c.z = a.z;
    }
  }
  I.color[pix] = c;
  if (I.count) I.count[pix] = make_float4(n, 0.0f, 0.0f, 0.0f);
}

}  // namespace

namespace urtd {

hipError_t launch_upsample(const UpsampleImages& I, const UpsampleSettings& P, hipStream_t st) {
  if (I.width <= 0 || I.height <= 0 || I.low_width <= 0 || I.low_height <= 0) return hipSuccess;
  const dim3 grid((unsigned int)((I.width + 15) / 16), (unsigned int)((I.height + 15) / 16));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_upsample, grid, dim3(256), 0, st, Params{I, P});
  return hipGetLastError();
}

}  // namespace urtd
