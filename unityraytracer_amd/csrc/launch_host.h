// launch_host.h — what the host-side launchers of the trace kernels share (kernels.hip and kernels_basic / _serve / _pool.hip, declared
// in kernels.h; query.hip, aov.hip, radiance.hip).  Included after the device headers, outside any namespace.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include "kernels.h"

namespace urtd {

static inline int blocks_for_tiles(const FrameParams& P) {
  int waves = P.block_threads / 64;
  int ntiles = P.tiles_x * P.n_strips;
  int nblocks = (ntiles + waves - 1) / waves;
  int q = 8 * P.xcd_run;                      // the block permutation of tile_pixel() acts on windows of 8*G blocks
  return ((nblocks + q - 1) / q) * q;
}

// Dynamic LDS of a workgroup whose lanes each keep the two traversal stacks of trace_device.h lane_stacks
static inline size_t stack_lds_bytes(LaneStackSize E, int block_threads) {
  return (size_t)(E.tlas + E.blas) * 64 * (size_t)(block_threads / 64) * sizeof(int);
}
static inline size_t stack_lds_bytes(const FrameParams& P) { return stack_lds_bytes({P.tlas_stack, P.blas_stack}, P.block_threads); }

// Names the trace launch *rec describes (urt_debug_launch_info): the kernel instantiation by the name rocprofv3 prints for it
static TraceLaunchRecord* named(TraceLaunchRecord* rec, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static TraceLaunchRecord* named(TraceLaunchRecord* rec, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt);
  vsnprintf(rec->kernel, sizeof rec->kernel, fmt, ap);
  va_end(ap);
  return rec;
}
static const char* tf(bool b) { return b ? "true" : "false"; }

// Dynamic LDS above the default 64 KiB per workgroup (very deep BVHs) raises the kernel's limit before its launch
static inline hipError_t raise_lds_limit(const void* kernel, size_t lds) {
  return lds > 64 * 1024 ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

// One trace-kernel launch; *rec (named by the caller) receives the grid and the dynamic LDS
template <typename... KP, typename... A>
static hipError_t launch_traced(TraceLaunchRecord* rec, void (*kernel)(KP...), int n_blocks, int block_threads, size_t lds, hipStream_t st,
                                const A&... args) {
  hipError_t e = raise_lds_limit((const void*)kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(block_threads), lds, st, args...);
  rec->n_blocks = n_blocks; rec->block_threads = block_threads; rec->lds_bytes = (int)lds;
  return hipGetLastError();
}

// The persistent kernels (modes 2 - 5) draw their tiles from kWorkShards counters, one per 128-byte line: zeroed before every launch
static inline hipError_t reset_work_counters(unsigned int* next, hipStream_t st) {
  return hipMemsetAsync(next, 0, kWorkShards * 32 * sizeof(unsigned int), st);
}

// What a batched launch (modes 3 and 5: P.n_frames frames, front modes 0 - 2) asks of its arguments, whichever kernel runs it
static inline bool batched_args_ok(const DevScene& S, const FrameParams& P, int front_mode) {
  if (P.n_frames < 1 || P.n_frames > kMaxFramesPerLaunch) return false;
  return !(front_mode == 2 && (!P.lds_mesh || S.n_meshes > 12 || P.tlas_stack < 2));
}

}  // namespace urtd
