// hist_sweep.hip — the launch shape of urt_auto_exposure's kernels (csrc/tonemap.hip, included as it is): k_luminance_histogram and
// k_exposure_resolve timed with events over workgroups x unroll x accumulator copies, at 1920x1080 and 3840x2160, on the constant image
// (every texel in one bin) and on luminances spread log-uniformly over twelve stops; beside them a device-to-device copy of the image
// and the 1032-byte memset a version that accumulated in the caller's state needed per call.  Each line is the mean of 100 calls after
// 10, every case twice.  The log that chose 1024 workgroups, unroll 4 and 8 copies: profiles/r20_logs/hist_sweep.log.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I unityraytracer_amd/csrc -I include scripts/micro/hist_sweep.hip -o scripts/micro/hist_sweep
#include "../../unityraytracer_amd/csrc/tonemap.hip"
#include <cstdio>
#include <vector>
#include <cmath>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
template <int U>
static void launch(const float4* src, unsigned n, unsigned* accum, unsigned copies, unsigned blocks, urtd::ExposureState* st, hipStream_t s) {
  hipLaunchKernelGGL(k_luminance_histogram<U>, dim3(blocks), dim3(256), 0, s, src, (const float4*)nullptr, n, accum, copies);
  hipLaunchKernelGGL(k_exposure_resolve, dim3(1), dim3(256), 0, s, accum, copies, st, urtd::ExposureSettings{0.18f, 1.0f / 64, 64.0f, 1.0f, 100, 950});
}
int main() {
  hipStream_t s; CK(hipStreamCreate(&s));
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  unsigned* accum; CK(hipMalloc(&accum, 64 * 257 * 4)); CK(hipMemset(accum, 0, 64 * 257 * 4));
  urtd::ExposureState* st; CK(hipMalloc(&st, sizeof(urtd::ExposureState))); CK(hipMemset(st, 0, sizeof(urtd::ExposureState)));
  const int sizes[2][2] = {{1920, 1080}, {3840, 2160}};
  for (int si = 0; si < 2; si++) {
    const unsigned n = sizes[si][0] * sizes[si][1];
    for (int content = 0; content < 2; content++) {
      std::vector<float> h((size_t)n * 4);
      srand(7);
      for (unsigned i = 0; i < n; i++) {
        const float v = content == 0 ? 0.5f : exp2f(-6.0f + 12.0f * (float)rand() / (float)RAND_MAX);
        h[4 * (size_t)i] = h[4 * (size_t)i + 1] = h[4 * (size_t)i + 2] = v; h[4 * (size_t)i + 3] = 1.0f;
      }
      float4* src; CK(hipMalloc(&src, (size_t)n * 16)); CK(hipMemcpy(src, h.data(), (size_t)n * 16, hipMemcpyHostToDevice));
      float4* dst; CK(hipMalloc(&dst, (size_t)n * 16));
      float ms;
      for (int rep = 0; rep < 2; rep++) {
        for (int i = 0; i < 10; i++) CK(hipMemcpyAsync(dst, src, (size_t)n * 16, hipMemcpyDeviceToDevice, s));
        CK(hipEventRecord(a, s));
        for (int i = 0; i < 100; i++) CK(hipMemcpyAsync(dst, src, (size_t)n * 16, hipMemcpyDeviceToDevice, s));
        CK(hipEventRecord(b, s)); CK(hipEventSynchronize(b)); CK(hipEventElapsedTime(&ms, a, b));
        printf("%dx%d %s copy_d2d us=%.2f\n", sizes[si][0], sizes[si][1], content ? "spread" : "constant", ms * 10);
        for (int i = 0; i < 10; i++) CK(hipMemsetAsync(&st->counted, 0, 1032, s));
        CK(hipEventRecord(a, s));
        for (int i = 0; i < 100; i++) CK(hipMemsetAsync(&st->counted, 0, 1032, s));
        CK(hipEventRecord(b, s)); CK(hipEventSynchronize(b)); CK(hipEventElapsedTime(&ms, a, b));
        printf("%dx%d %s memset_1032 us=%.2f\n", sizes[si][0], sizes[si][1], content ? "spread" : "constant", ms * 10);
        for (unsigned blocks : {256u, 512u, 1024u, 2048u})
          for (unsigned copies : {1u, 8u, 64u})
            for (int unroll : {4, 8}) {
              auto go = [&]() { if (unroll == 4) launch<4>(src, n, accum, copies, blocks, st, s); else launch<8>(src, n, accum, copies, blocks, st, s); };
              for (int i = 0; i < 10; i++) go();
              CK(hipEventRecord(a, s));
              for (int i = 0; i < 100; i++) go();
              CK(hipEventRecord(b, s)); CK(hipEventSynchronize(b)); CK(hipEventElapsedTime(&ms, a, b));
              urtd::ExposureState hs; CK(hipMemcpy(&hs, st, sizeof hs, hipMemcpyDeviceToHost));
              printf("%dx%d %s blocks=%u copies=%u unroll=%d us=%.2f counted=%u\n", sizes[si][0], sizes[si][1], content ? "spread" : "constant", blocks,
                     copies, unroll, ms * 10, hs.counted);
            }
      }
      CK(hipFree(src)); CK(hipFree(dst));
    }
  }
  return 0;
}
