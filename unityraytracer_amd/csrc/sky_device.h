// sky_device.h — the sky lookup of Shade's miss branch (RS:420-427, A.11) that the frame kernels (shade_device.h shade_sky) and the
// feature buffers (aov.hip) share: the direction -> (u, v) math and the bilinear, repeat-wrapped texel fetch.  Internal to the library;
// included by .hip translation units only, after trace_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"

using namespace urt;
using namespace urtd;

namespace {

__device__ __forceinline__ v3 sample_sky(const DevScene& S, float u, float v) {
  int W = S.sky_w, H = S.sky_h;
  float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
  float x0f = f_floor(x), y0f = f_floor(y);
  float fx = x - x0f, fy = y - y0f;
  int x0 = (int)x0f, y0 = (int)y0f;
  // repeat wrap.  The sky lookup's (u, v) lie in [-0.5, 0.5] x [-1, 0] (RS:424-425), so the texel index is within one period of the image:
  // one conditional add gives what the integer modulo (two dozen instructions each) gives; anything else takes the modulo
#ifndef URT_SKY_FASTWRAP
#define URT_SKY_FASTWRAP 1
#endif
  if (URT_SKY_FASTWRAP && (unsigned)x0 + (unsigned)W < 2u * (unsigned)W && (unsigned)y0 + (unsigned)H < 2u * (unsigned)H) {
    if (x0 < 0) x0 += W;
    if (y0 < 0) y0 += H;
  } else {
    x0 %= W; if (x0 < 0) x0 += W;
    y0 %= H; if (y0 < 0) y0 += H;
  }
  int x1 = x0 + 1; if (x1 == W) x1 = 0;
  int y1 = y0 + 1; if (y1 == H) y1 = 0;
  float4 c00 = S.sky[(size_t)y0 * W + x0], c10 = S.sky[(size_t)y0 * W + x1];
  float4 c01 = S.sky[(size_t)y1 * W + x0], c11 = S.sky[(size_t)y1 * W + x1];
  float ax = f_fma(fx, c10.x - c00.x, c00.x), bx = f_fma(fx, c11.x - c01.x, c01.x);
  float ay = f_fma(fx, c10.y - c00.y, c00.y), by = f_fma(fx, c11.y - c01.y, c01.y);
  float az = f_fma(fx, c10.z - c00.z, c00.z), bz = f_fma(fx, c11.z - c01.z, c01.z);
  return mk3(f_fma(fy, bx - ax, ax), f_fma(fy, by - ay, ay), f_fma(fy, bz - az, az));
}

// The sky radiance Shade returns for a ray that hit nothing (RS:424-426).
__device__ __forceinline__ v3 sky_radiance(const DevScene& S, v3 d) {
  // RS:424-425 divide by the constant -PI: f_div_const (urt_math.h) = the IEEE quotient for every float (exhaustive test), ten
  // instructions fewer per division; the oracle keeps the divider
  float theta = f_div_const(f_acos(d.y), -kPI, 1.0f / -kPI);
  float phi = f_div_const(f_atan2(d.x, -d.z), -kPI, 1.0f / -kPI) * 0.5f;
  return sample_sky(S, phi, theta);
}

}  // namespace
