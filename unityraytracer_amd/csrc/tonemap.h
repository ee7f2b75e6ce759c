// tonemap.h — host-callable launchers of the auto-exposure and tone-mapping kernels (tonemap.hip): urt_auto_exposure, urt_tonemap
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace urtd {

constexpr int kExposureBins = 256;         // include/urt.h urt_ExposureState.hist
constexpr int kExposureMaxBlocks = 1024;   // the histogram's grid is capped here (x 256 lanes); the rest of the image is grid-strided
constexpr int kExposureCopies = 8;         // accumulators in the context's scratch the workgroups flush to, round-robin
constexpr int kExposureWords = kExposureBins + 1;   // one accumulator: the bins, then the skipped texels

// include/urt.h urt_ExposureState, 1040 bytes, in caller-owned device memory
struct ExposureState {
  float exposure, target;
  uint32_t counted, skipped;
  uint32_t hist[kExposureBins];
};

// include/urt.h urt_ExposureParams, already checked
struct ExposureSettings {
  float key, min_exposure, max_exposure, rate;
  int low_permille, high_permille;
};

// include/urt.h urt_TonemapParams, already checked
struct TonemapSettings {
  float exposure, white;
  int op;                                  // URT_TONEMAP_*
};

// Enqueues on `st`: k_luminance_histogram over n_texels RGBA32F texels of src (and of count, when given) and k_exposure_resolve.
// accum: kExposureCopies * kExposureWords words of device scratch, ALL ZERO when the call is enqueued; the resolve leaves them zero
// again.  n_texels <= 2^31 - 1 (hipErrorInvalidValue otherwise).
hipError_t launch_auto_exposure(const float4* src, const float4* count, size_t n_texels, const ExposureSettings& P, unsigned int* accum,
                                ExposureState* state, hipStream_t st);

// Enqueues k_tonemap on `st`: dst[i] = operator(src[i] * e), alpha copied; e from P.exposure and, when state is given, its exposure.
// dst may be src.
hipError_t launch_tonemap(const float4* src, float4* dst, size_t n_texels, const TonemapSettings& P, const ExposureState* state,
                          hipStream_t st);

}  // namespace urtd
