// frame_derived.h — what every pixel of a frame derives from the frame's uniforms alone, computed once on the host when the frame enters
// a batched launch's table (frame_batch.cpp) instead of per lane at every refill of the trace kernel (frame_device.h camera_ray_frame):
// the seed-only halves of the pixel's first two rand() draws (RS:448-449, seeds _Seed and _Seed + 0.5) and the camera ray's origin
// (RS:145).  The very functions of include/urt_math.h on the same operands: the values are the per-lane ones bit for bit
// (tests/test_uniform_refill_host.py).  No HIP in here: host code, also compiled into a stand-alone test program.
#pragma once
#include "../../include/urt_math.h"

namespace urtd {

struct FrameDerived {
  float a0;                 // rand_scale(_Seed): the multiplier of the pixel's first draw
  float a1;                 // rand_scale(_Seed + 0.5f): of its second
  float origin[3];          // mul(_CameraToWorld, float4(0, 0, 0, 1)).xyz
};

inline FrameDerived frame_derived(const float* c2w, float seed) {
  FrameDerived d;
  d.a0 = urt::rand_scale(seed);
  d.a1 = urt::rand_scale(seed + 0.5f);
  const urt::v3 o = urt::mul_m4(c2w, 0.0f, 0.0f, 0.0f, 1.0f);
  d.origin[0] = o.x; d.origin[1] = o.y; d.origin[2] = o.z;
  return d;
}

}  // namespace urtd
