// object_bvh.hip — the object-level BVH on the device (include/urt.h "the object-level BVH on the device"):
//   k_mesh_leaf_partial / k_mesh_leaf_final   the world-space box of every MeshObject over the vertices its index slots name
//   k_sphere_leaves                           the box of every sphere
//   k_object_heap                             the implicit heap of csrc/host_scene.cpp urt_host_build_object_bvh, one workgroup
// The results equal the host functions by value (include/urt.h states when): float32, one rounding per operation, evaluated as written,
// no fma — built with -ffp-contract=off like every normative kernel.  No atomics, and no workgroup waits for another.
#include "experiments.h"

#include "object_bvh.h"

#include <algorithm>

#include "bounds_device.h"

namespace {

using namespace urtd;

constexpr int kMeshObjectWords = 28, kSphereWords = 14, kNodeWords = 7;   // 112, 56 and 28 bytes (include/urt_types.h)

// The index range of MeshObject m as the kernels use it: count 0 unless the whole range lies inside _Indices (the call has validated
// it on the host copy; a range that does not fit is never followed).
__device__ __forceinline__ void mesh_range(const float* __restrict__ mo, int n_indices, int& off, int& cnt) {
  off = __float_as_int(mo[16]); cnt = __float_as_int(mo[17]);
  if (off < 0 || cnt < 0 || (long long)off + (long long)cnt > (long long)n_indices) cnt = 0;
}

__device__ __forceinline__ int mesh_blocks(int cnt) { return min(kMeshLeafBlocks, (cnt + 255) >> 8); }

// Grid (kMeshLeafBlocks, n_meshes): the first mesh_blocks(count) workgroups of row m stride over mesh m's slots, the others leave at once
// (mesh sizes differ by orders of magnitude).  Index slots are read coalesced, each vertex is gathered as three dwords and transformed;
// a slot whose index lies outside the vertices is skipped.  One partial per workgroup.
__global__ __launch_bounds__(256) void k_mesh_leaf_partial(const float* __restrict__ mesh_objects, const float* __restrict__ vertices,
                                                           int n_vertices, const int32_t* __restrict__ indices, int n_indices,
                                                           float* __restrict__ partial) {
  const int m = (int)blockIdx.y;
  const float* mo = mesh_objects + (size_t)m * kMeshObjectWords;
  int off, cnt;
  mesh_range(mo, n_indices, off, cnt);
  const int nb = mesh_blocks(cnt);
  if ((int)blockIdx.x >= nb) return;                       // uniform over the workgroup
  float M[12];                                             // rows 0..2 of the four columns: M[3*c + r] = matrix[4*c + r]
  for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) M[3 * c + r] = mo[4 * c + r];
  Bounds b = empty_bounds();
  for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < (unsigned int)cnt; i += (unsigned int)nb * 256u) {   // < 2^31 + 2^16: no wrap
    const int vi = indices[(size_t)off + (size_t)i];
    if ((unsigned int)vi >= (unsigned int)n_vertices) continue;
    const size_t at = (size_t)vi * 3;
    const float px = vertices[at], py = vertices[at + 1], pz = vertices[at + 2];
    float w[3];
    for (int r = 0; r < 3; r++) w[r] = ((M[r] * px + M[3 + r] * py) + M[6 + r] * pz) + M[9 + r];
    join(b, w, w, 1u);
  }
  reduce_and_store(b, partial + ((size_t)m * kMeshLeafBlocks + blockIdx.x) * kMeshLeafWords);
}

// One workgroup per MeshObject: the union of its partials, written as its 28-byte leaf.
__global__ __launch_bounds__(256) void k_mesh_leaf_final(const float* __restrict__ mesh_objects, int n_indices, const float* __restrict__ partial,
                                                         int first_mesh, float* __restrict__ leaves) {
  const int m = (int)blockIdx.x;
  int off, cnt;
  mesh_range(mesh_objects + (size_t)m * kMeshObjectWords, n_indices, off, cnt);
  const int nb = mesh_blocks(cnt);
  Bounds b = empty_bounds();
  for (int i = (int)threadIdx.x; i < nb; i += 256) {
    const float* p = partial + ((size_t)m * kMeshLeafBlocks + i) * kMeshLeafWords;
    join(b, p, p + 3, __float_as_uint(p[6]));
  }
  const Bounds r = reduce_block(b);
  if (threadIdx.x == 0) {
    float* o = leaves + (size_t)m * kNodeWords;
    for (int c = 0; c < 3; c++) { o[c] = cnt > 0 ? r.lo[c] : 0.0f; o[3 + c] = cnt > 0 ? r.hi[c] : 0.0f; }
    o[6] = __int_as_float(first_mesh + m);
  }
}

// One sphere per lane.
__global__ __launch_bounds__(256) void k_sphere_leaves(const float* __restrict__ spheres, int n, float* __restrict__ leaves) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const float* s = spheres + (size_t)i * kSphereWords;
  const float radius = s[3];
  float* o = leaves + (size_t)i * kNodeWords;
  for (int k = 0; k < 3; k++) {
    const float a = s[k] - (-radius), b = s[k] - radius;
    o[k] = b < a ? b : a;                                  // std::min(a, b), std::max(a, b)
    o[3 + k] = a < b ? b : a;
  }
  o[6] = __int_as_float(i);
}

// A key's place in the total order of the centres: values as floats compare (-0 = +0), every NaN above +inf.
__device__ __forceinline__ unsigned int order_key(unsigned int u) {
  const unsigned int mag = u & 0x7fffffffu;
  if (mag == 0u) u = 0u;
  else if (mag > 0x7f800000u) u = 0x7fc00000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned int pick(const uint4& it, int ax) { return ax == 0 ? it.x : (ax == 1 ? it.y : it.z); }

// The number of leaves below heap slot s of level d (s = 2^d - 1 + t), 0 when the slot lies below a leaf: the median split's topology
// depends on n alone.
__device__ __forceinline__ int slot_count(int s, int d, int n) {
  int cnt = n;
  const unsigned int path = (unsigned int)s + 1u;          // below its leading one: the d turns from the root, 1 = right
  for (int bit = d - 1; bit >= 0; bit--) {
    if (cnt < 2) return 0;
    const int half = (cnt + 1) >> 1;
    cnt = ((path >> bit) & 1u) ? cnt - half : half;
  }
  return cnt;
}

// ONE workgroup, lane p owns POSITION p of the item list (p < n <= kObjectBvhDeviceMax).  items[p] = the three centre keys (float bits)
// and the leaf number of the item that stands at p now.  The segment [lo, hi) and the heap slot that position p belongs to at each level
// follow from n alone; only the permutation depends on the boxes.  Per level every lane of a segment of two or more finds the centre
// extents of its segment, the axis, and its item's rank under (key, leaf number) by counting — sum over the levels ~ 2 n reads of 16
// bytes per lane, all lanes of a segment reading the same address (a broadcast) — and the items move to lo + rank.  A segment of one
// copies its leaf record.  The interior boxes are then joined bottom-up from the children's records, one lane per node: min and max are
// exact, so this is the host's union over the leaves.  `nodes` is written and read back by this workgroup only, across barriers.
__global__ __launch_bounds__(kObjectBvhDeviceMax) void k_object_heap(const float* __restrict__ leaves, int n, float* nodes, int len, int depth) {
  __shared__ uint4 items[kObjectBvhDeviceMax];
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  for (int i = tid; i < len; i += nt) {                    // filler: all zero, index -1
    float* o = nodes + (size_t)i * kNodeWords;
    for (int k = 0; k < 6; k++) o[k] = 0.0f;
    o[6] = __int_as_float(-1);
  }
  const bool live = tid < n;
  if (live) {
    const float* l = leaves + (size_t)tid * kNodeWords;
    uint4 it;
    it.x = __float_as_uint(0.5f * l[0] + 0.5f * l[3]);
    it.y = __float_as_uint(0.5f * l[1] + 0.5f * l[4]);
    it.z = __float_as_uint(0.5f * l[2] + 0.5f * l[5]);
    it.w = (unsigned int)tid;
    items[tid] = it;
  }
  __syncthreads();
  int slot = 0, lo = 0, hi = n;
  bool placed = false;
  for (int d = 0; d < depth; d++) {
    const int cnt = hi - lo;
    const bool split = live && cnt >= 2;
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    int dest = tid;
    if (live && cnt == 1 && !placed) {                     // a one-object range keeps its leaf record verbatim
      const float* l = leaves + (size_t)items[tid].w * kNodeWords;
      float* o = nodes + (size_t)slot * kNodeWords;
      for (int k = 0; k < kNodeWords; k++) o[k] = l[k];
      placed = true;
    }
    if (split) {
      const float inf = __builtin_inff();
      float clo[3] = {inf, inf, inf}, chi[3] = {-inf, -inf, -inf};
      for (int q = lo; q < hi; q++) {
        const uint4 it = items[q];
        const float c[3] = {__uint_as_float(it.x), __uint_as_float(it.y), __uint_as_float(it.z)};
        for (int k = 0; k < 3; k++) { clo[k] = c[k] < clo[k] ? c[k] : clo[k]; chi[k] = chi[k] < c[k] ? c[k] : chi[k]; }
      }
      int ax = 0;
      float ext = chi[0] - clo[0];
      const float e1 = chi[1] - clo[1], e2 = chi[2] - clo[2];
      if (e1 > ext) { ax = 1; ext = e1; }
      if (e2 > ext) ax = 2;
      mine = items[tid];
      const unsigned int my_key = order_key(pick(mine, ax)), my_leaf = mine.w;
      int rank = 0;
      for (int q = lo; q < hi; q++) {
        const uint4 it = items[q];
        const unsigned int key = order_key(pick(it, ax));
        rank += (key < my_key || (key == my_key && it.w < my_leaf)) ? 1 : 0;
      }
      dest = lo + rank;                                    // a permutation of [lo, hi): the order is total, the leaf numbers differ
    }
    __syncthreads();
    if (split) items[dest] = mine;
    __syncthreads();
    if (split) {
      const int half = (cnt + 1) >> 1;
      if (tid < lo + half) { slot = 2 * slot + 1; hi = lo + half; }
      else { slot = 2 * slot + 2; lo = lo + half; }
    }
  }
  for (int d = depth - 2; d >= 0; d--) {
    __syncthreads();                                       // the records of level d + 1 are written
    for (int t = tid; t < (1 << d); t += nt) {
      const int s = (1 << d) - 1 + t;
      if (slot_count(s, d, n) < 2) continue;               // a leaf, or a filler below one
      const float* a = nodes + (size_t)(2 * s + 1) * kNodeWords;
      const float* b = nodes + (size_t)(2 * s + 2) * kNodeWords;
      float* o = nodes + (size_t)s * kNodeWords;
      for (int k = 0; k < 3; k++) {
        const float a0 = a[k], a1 = a[3 + k], b0 = b[k], b1 = b[3 + k];
        const float alo = a1 < a0 ? a1 : a0, ahi = a0 < a1 ? a1 : a0, blo = b1 < b0 ? b1 : b0, bhi = b0 < b1 ? b1 : b0;
        o[k] = blo < alo ? blo : alo;
        o[3 + k] = ahi < bhi ? bhi : ahi;
      }
      o[6] = __int_as_float(-1);
    }
  }
}

}  // namespace

namespace urtd {

hipError_t mesh_leaf_bounds(const char* mesh_objects, int n_meshes, const float* vertices, int n_vertices, const int32_t* indices,
                            int n_indices, float* partial, char* leaves, hipStream_t st) {
  constexpr int kRows = 65535;                             // gridDim.y; `partial` serves one launch pair after the other, in stream order
  for (int first = 0; first < n_meshes; first += kRows) {
    const int rows = std::min(kRows, n_meshes - first);
    const float* mo = (const float*)(mesh_objects + (size_t)first * 112);
    hipLaunchKernelGGL(k_mesh_leaf_partial, dim3(kMeshLeafBlocks, rows), dim3(256), 0, st, mo, vertices, n_vertices, indices, n_indices, partial);
    hipLaunchKernelGGL(k_mesh_leaf_final, dim3(rows), dim3(256), 0, st, mo, n_indices, (const float*)partial, first,
                       (float*)(leaves + (size_t)first * 28));
  }
  return hipGetLastError();
}

hipError_t sphere_leaf_bounds(const char* spheres, int n, char* leaves, hipStream_t st) {
  hipLaunchKernelGGL(k_sphere_leaves, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, st, (const float*)spheres, n, (float*)leaves);
  return hipGetLastError();
}

hipError_t build_object_bvh(const char* leaves, int n, char* nodes, int len, hipStream_t st) {
  int depth = 1;
  while ((1 << (depth - 1)) < n) depth++;                  // len = 2^depth - 1
  const int threads = std::min(kObjectBvhDeviceMax, std::max(64, (n + 63) & ~63));
  hipLaunchKernelGGL(k_object_heap, dim3(1), dim3(threads), 0, st, (const float*)leaves, n, (float*)nodes, len, depth);
  return hipGetLastError();
}

}  // namespace urtd
