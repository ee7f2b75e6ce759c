// tile_entry.hip — the pre-pass that builds the tile entry table (tile_entry.h): one thread per 8x8 tile of the image walks the common
// part of its camera rays' BVH descent and writes the tile's record, kTileEntryK dwords.  Run once per (camera, image size, node
// contents) on the stream of the trace launch that needs it (frame_batch.cpp); a 1080p image has 32,400 tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "tile_entry.h"

namespace {

struct TileCamera { float c2w[16], invp[16]; };

__global__ __launch_bounds__(64) void k_tile_entry(urtd::DevScene S, int n_nodes, TileCamera cam, int width, int height, int tiles_x, int tiles_y,
                                                   int32_t* __restrict__ table) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tiles_x * tiles_y) return;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  // the one MeshObject the plain single-mesh FRONT enters (front_device.h front_single): the index of heap node 0
  int32_t root = urtd::kTileEntryDone;
  if (S.n_mesh_tlas > 0 && S.n_meshes > 0) {
    const int index = __builtin_bit_cast(int, S.mesh_tlas[0].w);
    if (index >= 0 && index < S.n_meshes) root = S.mesh_root[index];
  }
  int32_t e[urtd::kTileEntryK], rec[urtd::kTileEntryK];
  int n = 1;
  e[0] = root;
  if (root >= 0 && root < n_nodes) {
    const urtd::TileFrustum F = urtd::tile_frustum(cam.c2w, cam.invp, tx, ty, width, height);
    n = urtd::tile_entry_list((const float*)S.blas_cnodes, n_nodes, root, F, urtd::kTileEntryK, e);
  }
  urtd::tile_entry_record(e, n, urtd::kTileEntryK, rec);
  int4* dst = (int4*)(table + (size_t)t * urtd::kTileEntryK);
  for (int i = 0; i < urtd::kTileEntryK / 4; i++) dst[i] = make_int4(rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3]);
}

}  // namespace

namespace urtd {

hipError_t launch_tile_entry(const DevScene& S, int n_nodes, const float* c2w, const float* invp, int width, int height, int32_t* table, hipStream_t st) {
  const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
  if (tiles_x <= 0 || tiles_y <= 0) return hipSuccess;
  if (!S.blas_cnodes || !S.mesh_tlas || !S.mesh_root || !table) return hipErrorInvalidValue;
  TileCamera cam;
  for (int i = 0; i < 16; i++) { cam.c2w[i] = c2w[i]; cam.invp[i] = invp[i]; }
  const int n = tiles_x * tiles_y;
  hipLaunchKernelGGL(k_tile_entry, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, S, n_nodes, cam, width, height, tiles_x, tiles_y, table);
  return hipGetLastError();
}

}  // namespace urtd
