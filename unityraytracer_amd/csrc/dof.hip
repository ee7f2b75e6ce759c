// dof.hip — image-space depth of field ahead of the bloom (urt_depth_of_field): every pixel gets the blur radius of a thin lens from its
// hit distance, and gathers the pixels around it whose own blur reaches it.  include/urt.h states the arithmetic; the library is built
// with -ffp-contract=off, so every float expression below is evaluated with one rounding per operation, in the order written there.
// Division is IEEE, the only square roots are f_sqrt's of the distance table.  Both kernels run 256-thread workgroups over 16 x 16
// pixels, four waves of 8 x 8 as csrc/bloom.hip lays them out.
//
// k_dof_coc      one pixel per lane: its class and blur radius, {a, z} into the scratch (a pass-through pixel: a = 0, which no lens
//                pixel has), the tile's largest a into the tile table.  With URT_DOF_FLAG_COC it also writes dst, and nothing follows.
// k_dof_gather   one workgroup per tile.  A tap q counts for p only while d < a_q + 0.5 (include/urt.h "how far an implementation
//                looks"), so no tap further than R = ceil(M - 0.5) along an axis counts, M the largest a of the region the taps come
//                from.  Every tap of the tile lies in its 3 x 3 tile neighbourhood (a reach of 16 never leaves the adjacent tiles), so M is
//                the largest of nine table entries: wave-uniform, and the bound of the dy / dx loops.  M - 0.5 is exact for M in
//                [0.5, 16] (M + 0.5 is not: 15.5 + 2^-20 would round to 16 and lose the column 16 away).  The footprint, the tile and R
//                texels on each side, is staged once in LDS: colour and a as one float4, z beside it; pass-through pixels and texels
//                outside the image are staged with a = 0 and fail the tap's validity test (no clamping).  At R = 16 that is 48 x 48
//                texels, 52 KB of the CU's 160 KB with the rows' padding (below): three workgroups a CU, which the tap loop at that
//                reach does not need more of — but static LDS is paid at any R, and a short loop is latency bound.  a <= max_radius,
//                which the host knows, so the kernel is a template on the reach its LDS is sized for, 4, 8 or 16 (11, 20 and 52 KB: 8, 7
//                and 3 waves a SIMD), and the launch takes the smallest that holds ceil(max_radius - 0.5): at max_radius = 8 the gather
//                of an in-focus image takes 0.019 ms instead of 0.034 and that of the C3 frame 0.058 instead of 0.093
//                (profiles/r27_logs/dof_bench.log: product against libdof_lds48).  d comes from a table of |dy|, |dx| that every
//                workgroup fills with f_sqrt, (R + 1)^2 entries ahead of the barrier it needs anyway; no square root per tap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dof.h"
#include "../../include/urt_math.h"

namespace {

using urtd::DofSettings;
using urtd::kDofMaxReach;
using urt::bits_f;
using urt::f_bits;
using urt::f_sqrt;

constexpr int kTile = 16;
constexpr float kMaxColor = 0x1p100f;              // include/urt.h: a colour beyond it passes through

struct Texel2 { int x, y; };
__device__ __forceinline__ Texel2 tile_texel() {   // 16 x 16 texels a workgroup, 8 x 8 a wave
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  return {(wave & 1) * 8 + (lane & 7), (wave >> 1) * 8 + (lane >> 3)};
}

// (no __restrict__ on dst: it is written only with the flag, and then it is no input)
__global__ __launch_bounds__(256) void k_dof_coc(const float4* __restrict__ src, const float4* __restrict__ hit, float2* __restrict__ coc,
                                                 float* __restrict__ tile_max, float4* dst, int w, int h, const DofSettings P) {
  __shared__ unsigned int largest;                 // the bits of the tile's largest a (a >= 0: the order of the bits is the order of the floats)
  if (threadIdx.x == 0) largest = 0u;
  __syncthreads();
  const Texel2 l = tile_texel();
  const int x = (int)blockIdx.x * kTile + l.x, y = (int)blockIdx.y * kTile + l.y;
  if (x < w && y < h) {
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    const float4 c = src[i];
    const float z = hit[i].w;
    // (NaN fails every comparison)
    const bool lens = z > 0.0f && fabsf(c.x) <= kMaxColor && fabsf(c.y) <= kMaxColor && fabsf(c.z) <= kMaxColor;
    float a = 0.0f;
    if (lens) {
      a = fmaxf(fminf(fabsf(P.scale * (1.0f - P.focus_distance / z)), P.max_radius), 0.5f);
      atomicMax(&largest, f_bits(a));
    }
    coc[i] = make_float2(a, z);
    if (P.flags & 1) dst[i] = make_float4(a, a, a, c.w);
  }
  __syncthreads();
  if (threadIdx.x == 0) tile_max[(size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x] = bits_f(largest);
}

// kReach: the furthest any tile of the call can look, ceil(max_radius - 0.5) rounded up to 4, 8 or 16 — it sizes the LDS
template <int kReach>
__global__ __launch_bounds__(256) void k_dof_gather(const float4* __restrict__ src, const float2* __restrict__ coc,
                                                    const float* __restrict__ tile_max, float4* __restrict__ dst, int w, int h) {
  constexpr int kSide = kTile + 2 * kReach;        // the footprint's side at the full reach
  // The stride of the footprint's rows in LDS, in texels.  A ds_read_b128 is served in groups of 16 lanes that span four rows of the
  // 8 x 8 wave (a half of each); with rows a multiple of 256 B apart (the sides 48 and 32), two of those rows start on
  // the same banks: a 2-way conflict on the loop's main read.  An odd multiple of 128 B puts the four on four different quarters of
  // the 64 banks.  At the side 48 a stride of 56 still leaves three workgroups a CU and measured 1.6 % faster at the full reach; at
  // the side 32 a stride of 40 takes the seventh workgroup and measured 1.5 - 3 % slower, so those rows stay 32 apart; 24 is odd
  // already.  z (ds_read_b32: 32 lanes, four whole rows over 32 banks) keeps the side as its stride: 56 there would cost the third
  // workgroup at the side 48 (profiles/r27_logs/dof_bench.log: product against libdof_unpadded and libdof_padded8).
  constexpr int kFootStride = kReach == kDofMaxReach ? kSide + 8 : kSide;
  constexpr int kDepthStride = kSide;
  __shared__ float4 foot[kSide * kFootStride];     // (r, g, b, a) of the footprint's texels; a = 0: no tap
  __shared__ float depth[kSide * kDepthStride];    // z beside it
  __shared__ float dist[kReach + 1][kReach + 1];   // [|dy|][|dx|]

  const int bx = (int)blockIdx.x, by = (int)blockIdx.y, tx = (int)gridDim.x, ty = (int)gridDim.y;
  float M = 0.0f;                                  // the largest a of the 3 x 3 tile neighbourhood (uniform)
  for (int j = max(by - 1, 0); j <= min(by + 1, ty - 1); j++)
    for (int i = max(bx - 1, 0); i <= min(bx + 1, tx - 1); i++) M = fmaxf(M, tile_max[(size_t)j * (size_t)tx + (size_t)i]);
  const int R = __builtin_amdgcn_readfirstlane(min(max((int)ceilf(M - 0.5f), 0), kReach));   // (M <= max_radius: the min never bites)

  for (int i = threadIdx.x; i < (R + 1) * (R + 1); i += 256) {
    const int r = i / (R + 1), c = i - r * (R + 1);
    dist[r][c] = f_sqrt((float)(c * c + r * r));
  }
  const int side = kTile + 2 * R, x0 = bx * kTile - R, y0 = by * kTile - R;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int r = i / side, c = i - r * side;
    const int gx = x0 + c, gy = y0 + r;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float z = 0.0f;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {  // the image border is a validity test on the tap
      const size_t g = (size_t)gy * (size_t)w + (size_t)gx;
      const float2 az = coc[g];
      if (az.x > 0.0f) {
        const float4 s = src[g];
        t = make_float4(s.x, s.y, s.z, az.x);
        z = az.y;
      }
    }
    foot[r * kFootStride + c] = t;
    depth[r * kDepthStride + c] = z;
  }
  __syncthreads();

  const Texel2 l = tile_texel();
  const int x = bx * kTile + l.x, y = by * kTile + l.y;
  if (x >= w || y >= h) return;                    // (after the last barrier)
  const size_t i = (size_t)y * (size_t)w + (size_t)x;
  float4 p = src[i];
  const int own = (l.y + R) * kFootStride + (l.x + R), zown = (l.y + R) * kDepthStride + (l.x + R);
  const float ap = foot[own].w, zp = depth[zown];
  if (ap > 0.0f) {                                 // a lens pixel; a pass-through pixel keeps its bits
    float S = 0.0f, Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
    for (int dy = -R; dy <= R; dy++) {
      const float* const drow = dist[abs(dy)];
      const int row = own + dy * kFootStride, zrow = zown + dy * kDepthStride;
      for (int dx = -R; dx <= R; dx++) {
        const float4 q = foot[row + dx];
        if (!(q.w > 0.0f)) continue;
        const float ae = depth[zrow + dx] > zp ? fminf(q.w, ap) : q.w;
        const float cov = fminf(fmaxf((ae - drow[abs(dx)]) + 0.5f, 0.0f), 1.0f);
        if (!(cov > 0.0f)) continue;               // skipped, not added as zero
        const float wq = cov / (ae * ae);
        S = S + wq;
        Ar = Ar + wq * q.x;
        Ag = Ag + wq * q.y;
        Ab = Ab + wq * q.z;
      }
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

hipError_t launch_depth_of_field(const float4* src, const float4* hit, float4* dst, int width, int height, const DofSettings& P,
                                 float* scratch, hipStream_t st) {
  if (width < 1 || height < 1 || width > kDofMaxExtent || height > kDofMaxExtent || (height + 15) / 16 > 65535) return hipErrorInvalidValue;
  float2* const coc = (float2*)scratch;
  float* const tile_max = scratch + 2 * (size_t)width * (size_t)height;
  hipLaunchKernelGGL(k_dof_coc, tiles(width, height), dim3(256), 0, st, src, hit, coc, tile_max, dst, width, height, P);
  if (!(P.flags & 1)) {
    const int reach = (int)ceilf(P.max_radius - 0.5f);            // a <= max_radius, so no tile's R is larger
    auto* const gather = reach <= 4 ? k_dof_gather<4> : reach <= 8 ? k_dof_gather<8> : k_dof_gather<kDofMaxReach>;
    hipLaunchKernelGGL(gather, tiles(width, height), dim3(256), 0, st, src, (const float2*)coc, (const float*)tile_max, dst, width, height);
  }
  return hipGetLastError();
}

}  // namespace urtd
