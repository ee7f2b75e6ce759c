// resample.h — host-callable launchers of the resampling step (resample.hip): the ordered compaction of a count texture into a pixel list
// (urt_select_pixels) and the sparse AdditionShader blend of a sample list (urt_blend_samples)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace urtd {

// Texels one 256-thread workgroup of the selection kernels handles: four waves x kSelectRounds x 64 consecutive texels.
// (unity_api.SELECT_CHUNK states the same number for the tests that straddle a chunk boundary.)
constexpr int kSelectRounds = 8;
constexpr int kSelectChunk = 4 * 64 * kSelectRounds;   // 2048

// Workgroups (= per-block counts) the selection of n_texels texels uses.
inline size_t select_blocks(size_t n_texels) { return (n_texels + (size_t)kSelectChunk - 1) / (size_t)kSelectChunk; }

// Unsigned words of scratch the selection needs: one count per block, then the grand total.
inline size_t select_scratch_words(size_t n_texels) { return select_blocks(n_texels) + 1; }

// Phases 1 and 2: k_select_count writes the number of selected texels of every chunk to scratch[0 .. blocks), k_select_scan replaces them
// by their exclusive prefix sums and writes the grand total to scratch[blocks].  A texel is selected when !(count.x >= below).
// n_texels = width * height <= 2^31 - 1.
hipError_t launch_select_count(const float4* count, size_t n_texels, float below, unsigned int* scratch, hipStream_t st);

// Phase 3, after the two above on the same stream: the selected texels of rank < capacity are written to pixels[rank] as {x, y} in
// ascending texel order.  capacity <= 0: nothing is launched.
hipError_t launch_select_write(const float4* count, int width, size_t n_texels, float below, const unsigned int* scratch, int2* pixels,
                               int capacity, hipStream_t st);

// k_blend_samples: entry i blends samples[i] into dst / count at pixels[i] with the operations of include/urt.h "resampling"; an entry
// whose pixel lies outside width x height is skipped.
hipError_t launch_blend_samples(const int2* pixels, const float4* samples, int n, float weight, float4* dst, float4* count, int width,
                                int height, float max_history, hipStream_t st);

}  // namespace urtd
