// motion_blur.hip — image-space motion blur between the depth of field and the bloom (urt_motion_blur): every pixel gets the velocity
// of the open shutter from the motion image urt_reproject* writes, every 16 x 16 tile the velocity of its fastest pixel, and a pixel is
// gathered along the fastest velocity of its 3 x 3 tile neighbourhood.  include/urt.h states the arithmetic; the library is built with
// -ffp-contract=off, so every float expression below is evaluated with one rounding per operation, in the order written there.
// Division is IEEE, the square roots are f_sqrt's.  Both kernels run 256-thread workgroups over 16 x 16 pixels, lane t on the texel
// (t & 15, t >> 4) of the tile: a wave covers four rows of 16 texels, and the order of the lanes is the order of y * W + x.
//
// k_mb_velocity  one pixel per lane: its class and clamped velocity; {l, z} into the scratch (a pass-through pixel: l = -1, which no
//                moving pixel has); the tile's dominant pixel — the largest m, among equal m the lowest lane — by a (m, lane) key that
//                is reduced across the wave with shuffles and across the four waves through LDS.  No atomics: a workgroup owns its
//                tile.  The winning lane stores {v.x, v.y, m, 0}.
// k_mb_gather    one workgroup per tile.  Its prologue takes the 3 x 3 maximum of the tile table (nine 16-byte reads at addresses that
//                depend on blockIdx alone); n, M, every (dx, dy), the repeated-k test and d are the same for the whole tile, so a
//                tap is one shifted row-wise read of the scratch and one of src per wave, straight from global memory (a tile's 33
//                taps lie on a line, not in a square: a staged 48 x 48 footprint would load nine times what the line touches).  A
//                still tile (mn < 0.25) is a uniform branch that copies 16 bytes per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "motion_blur.h"
#include "../../include/urt_math.h"

namespace {

using urtd::MotionBlurSettings;
using urt::f_sqrt;

constexpr int kTile = 16;
constexpr float kMaxColor = 0x1p100f;              // include/urt.h: a colour beyond it passes through

// the better of two (m, lane) keys: the larger m, among equal m the lower lane (m is never NaN)
__device__ __forceinline__ void better(float& m, int& lane, float m2, int lane2) {
  if (m2 > m || (m2 == m && lane2 < lane)) { m = m2; lane = lane2; }
}

__global__ __launch_bounds__(256) void k_mb_velocity(const float4* __restrict__ src, const float4* __restrict__ motion,
                                                     const float4* __restrict__ hit, float4* __restrict__ tile_v, float2* __restrict__ tap,
                                                     int w, int h, float half_shutter, float R) {
  __shared__ float wave_m[4];
  __shared__ int wave_lane[4];
  const int t = (int)threadIdx.x;
  const int x = (int)blockIdx.x * kTile + (t & 15), y = (int)blockIdx.y * kTile + (t >> 4);
  float vx = 0.0f, vy = 0.0f, m = -2.0f;             // outside the image: below every pixel's key
  if (x < w && y < h) {
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    const float4 c = src[i];
    const float z = hit[i].w;
    // (NaN fails every comparison)
    const bool moving = z > 0.0f && fabsf(c.x) <= kMaxColor && fabsf(c.y) <= kMaxColor && fabsf(c.z) <= kMaxColor;
    float l = -1.0f;
    m = -1.0f;
    if (moving) {
      const float4 mv = motion[i];
      if (fabsf(mv.x) <= 3.40282347e38f && fabsf(mv.y) <= 3.40282347e38f && mv.z > 0.0f) {   // finite components, a valid vector
        vx = half_shutter * mv.x;
        vy = half_shutter * mv.y;
      }
      l = f_sqrt(vx * vx + vy * vy);
      if (l > R) {
        const float s = R / l;
        vx = vx * s;
        vy = vy * s;
      }
      vx = fminf(fmaxf(vx, -R), R);
      vy = fminf(fmaxf(vy, -R), R);
      m = vx * vx + vy * vy;
      l = f_sqrt(m);
    }
    tap[i] = make_float2(l, z);
  }
  float bm = m;
  int bl = t;
  for (int off = 32; off >= 1; off >>= 1) {
    const float om = __shfl_xor(bm, off, 64);
    const int ol = __shfl_xor(bl, off, 64);
    better(bm, bl, om, ol);
  }
  if ((t & 63) == 0) { wave_m[t >> 6] = bm; wave_lane[t >> 6] = bl; }
  __syncthreads();
  bm = wave_m[0];
  bl = wave_lane[0];
  for (int k = 1; k < 4; k++) better(bm, bl, wave_m[k], wave_lane[k]);
  // (the winner is inside the image: lane 0 always is, and its key beats every lane outside)
  if (t == bl) tile_v[(size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x] = make_float4(vx, vy, m, 0.0f);
}

// (no __restrict__ games needed on dst: it is none of the inputs)
__global__ __launch_bounds__(256) void k_mb_gather(const float4* __restrict__ src, const float4* __restrict__ tile_v,
                                                   const float2* __restrict__ tap, float4* __restrict__ dst, int w, int h, int flags) {
  const int bx = (int)blockIdx.x, by = (int)blockIdx.y, tx = (int)gridDim.x, ty = (int)gridDim.y;
  float nx = 0.0f, ny = 0.0f, mn = -2.0f;          // the neighbourhood's dominant velocity (uniform): dy ascending, dx ascending, the first of equals
  for (int j = max(by - 1, 0); j <= min(by + 1, ty - 1); j++)
    for (int i = max(bx - 1, 0); i <= min(bx + 1, tx - 1); i++) {
      const float4 v = tile_v[(size_t)j * (size_t)tx + (size_t)i];
      if (v.z > mn) { nx = v.x; ny = v.y; mn = v.z; }
    }
  const int t = (int)threadIdx.x;
  const int x = bx * kTile + (t & 15), y = by * kTile + (t >> 4);
  if (x >= w || y >= h) return;                    // (no barrier below)
  const size_t i = (size_t)y * (size_t)w + (size_t)x;
  float4 p = src[i];
  if (flags & 1) {                                 // URT_MOTION_BLUR_FLAG_VELOCITY
    dst[i] = make_float4(nx, ny, fmaxf(tap[i].x, 0.0f), p.w);
    return;
  }
  if (!(mn >= 0.25f)) {                            // a still tile: nothing within reach moves half a pixel
    dst[i] = p;
    return;
  }
  const float2 own = tap[i];
  if (own.x >= 0.0f) {                             // a moving pixel; a pass-through pixel keeps its bits
    const float lp = fmaxf(own.x, 0.5f), zp = own.y;
    const int M = (int)ceilf(fmaxf(fabsf(nx), fabsf(ny)));      // 1 .. 16
    const float fM = (float)M;
    float S = 0.0f, Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
    int pdx = 0x7fffffff, pdy = 0x7fffffff;
    for (int k = -M; k <= M; k++) {
      const int dx = (int)floorf(((float)k * nx) / fM + 0.5f), dy = (int)floorf(((float)k * ny) / fM + 0.5f);
      const bool repeated = dx == pdx && dy == pdy;
      pdx = dx;
      pdy = dy;
      if (repeated) continue;                      // (uniform)
      const float d = f_sqrt((float)(dx * dx + dy * dy));
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
      const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
      const float2 tq = tap[q];
      if (!(tq.x >= 0.0f)) continue;               // passes through: never a tap
      const float ae = tq.y < zp ? fmaxf(tq.x, 0.5f) : lp;
      const float cov = fminf(fmaxf(1.0f - d / ae, 0.0f), 1.0f);
      if (!(cov > 0.0f)) continue;                 // skipped, not added as zero
      const float wq = cov / ae;
      const float4 c = src[q];
      S = S + wq;
      Ar = Ar + wq * c.x;
      Ag = Ag + wq * c.y;
      Ab = Ab + wq * c.z;
    }
    p.x = Ar / S;
    p.y = Ag / S;
    p.z = Ab / S;
  }
  dst[i] = p;                                      // alpha: the bits that were loaded
}

dim3 tiles(int w, int h) { return dim3((unsigned int)((w + 15) / 16), (unsigned int)((h + 15) / 16)); }

}  // namespace

namespace urtd {

hipError_t launch_motion_blur(const float4* src, const float4* motion, const float4* hit, float4* dst, int width, int height,
                              const MotionBlurSettings& P, float* scratch, hipStream_t st) {
  if (width < 1 || height < 1 || width > kMotionBlurMaxExtent || height > kMotionBlurMaxExtent || (height + 15) / 16 > 65535)
    return hipErrorInvalidValue;
  float4* const tile_v = (float4*)scratch;
  float2* const tap = (float2*)(scratch + 4 * motion_blur_tiles(width, height));
  hipLaunchKernelGGL(k_mb_velocity, tiles(width, height), dim3(256), 0, st, src, motion, hit, tile_v, tap, width, height,
                     P.shutter * 0.5f, P.max_radius);
  hipLaunchKernelGGL(k_mb_gather, tiles(width, height), dim3(256), 0, st, src, (const float4*)tile_v, (const float2*)tap, dst, width, height,
                     P.flags);
  return hipGetLastError();
}

}  // namespace urtd
