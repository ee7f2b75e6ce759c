// refit.hip — GPU refit of the triangle BVHs of MOVED MeshObjects (dynamic scenes).
//
// The reference's protocol for a moving object is "re-upload everything" (RayTraceMaster.cs:215-230 -> 262-336: any
// Register/Unregister or transform change rebuilds all lists and calls SetData on all seven buffers).  When all that changed is the
// localToWorldMatrix of some MeshObjects, their triangle BVHs keep their TOPOLOGY (a good SAH tree stays a good tree under a rigid
// or affine motion): only the world-space triangle records (RS:244-246 applied once per upload) and the boxes have
// to follow.  Both are recomputed here, in place, on the GPU, from device-resident copies of _Vertices / _Indices:
//   k_refit_tris   one lane per leaf-order triangle of a moved MeshObject: the normative mul(localToWorld, float4(v, 1)) of its three
//                  vertices with the NEW matrix -> the 48-byte record (v0 | slot, e1 | mesh, e2 | 0) — bit-identical to what a full
//                  rebuild writes (blas_builder.cpp `records`) — and the MeshObject's largest |coordinate| (the box pad's scale);
//   k_refit_level  bottom-up, one launch per tree level: a node's two child boxes from the new records (leaf children) or from the
//                  level below (interior children), written with the builder's pad of 2^-16 x largest |coordinate| (blas_builder.cpp).
// A DEFORMED MeshObject (elements of _Vertices changed under an unchanged topology: skinning, cloth, blend shapes) takes the same two passes
// — the kernels do not distinguish a new matrix from new vertices — and two more exist for it:
//   k_refit_norms  one lane per leaf-order triangle of a MeshObject whose _Normals changed: its three object-space shading normals are
//                  gathered again into tri_norms, bit-identical to what blas_builder.cpp / lbvh.hip write at a build (RS:259-261);
//   k_tree_cost    the surface-area cost of every MeshObject's tree from the [lo, hi] nodes, so that the host can tell a tree that a large
//                  deformation has spoilt (scene_prep.cpp, option "refit_rebuild_pct").  It steers speed, never pixels.
// Which nodes belong to which MeshObject, every node's parent and its depth are derived once per full scene preparation (k_parents,
// k_node_mesh, k_depth) from the node array itself, so the refit works on trees of either builder (host SAH, GPU LBVH).
// The box rule: a leaf child's box is the min / max of the RECONSTRUCTED vertices r0, r0 + e1, r0 + e2 of its records (what the triangle
// test sees; not w1, w2), an interior child's box the unpadded union of the level below, and the pad (2^-16 x the largest finite
// |coordinate| of the node's OWN MeshObject + 1e-30) is added only where a box is written into a node.  Nodes of MeshObjects that did not
// move are not touched.  Pixels do not depend on the boxes only while they contain their triangles (they only cull; the Moller-Trumbore
// test decides): tests/refit_ref.py restates this rule, tests/test_refit_ref.py checks its margins, tests/test_gpu_refit_edges.py compares
// the refitted nodes with it bit for bit, and tests/test_gpu_refit.py compares moved scenes with a full rebuild and with the oracle.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "refit.h"

using namespace urt;

namespace {

__device__ __forceinline__ int as_i(float f) { return __builtin_bit_cast(int, f); }
__device__ __forceinline__ float as_f(int i) { return __builtin_bit_cast(float, i); }

__global__ __launch_bounds__(256) void k_parents(const float4* __restrict__ nodes, int n_nodes, int32_t* __restrict__ parent) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  float4 q3 = nodes[4 * (size_t)n + 3];
  int c0 = as_i(q3.x), c1 = as_i(q3.y);
  if (c0 >= 0 && c0 < n_nodes) parent[c0] = n;
  if (c1 >= 0 && c1 < n_nodes) parent[c1] = n;
}

// every node's MeshObject: a node with a leaf child reads it from that leaf's first triangle and hands it up its ancestor chain
// (all ancestors belong to the same MeshObject; concurrent walkers write the same value, a walker stops where another has been)
__global__ __launch_bounds__(256) void k_node_mesh(const float4* __restrict__ nodes, const float4* __restrict__ tri_verts, int n_nodes,
                                                   const int32_t* __restrict__ parent, int32_t* node_mesh) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  float4 q3 = nodes[4 * (size_t)n + 3];
  int c0 = as_i(q3.x), c1 = as_i(q3.y);
  int leaf = c0 < 0 ? c0 : c1;
  if (leaf >= 0) return;
  uint32_t first = (~(uint32_t)leaf) >> 3;
  int m = as_i(tri_verts[3 * (size_t)first + 1].w);
  for (int p = n; p >= 0; p = parent[p]) {
    if (__hip_atomic_load(&node_mesh[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == m) break;
    __hip_atomic_store(&node_mesh[p], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_refit_tris(float4* __restrict__ tri_verts, int n_tris, const float* __restrict__ vertices,
                                                    const int32_t* __restrict__ indices, const float* __restrict__ matrices,
                                                    const int32_t* __restrict__ moved, unsigned int* __restrict__ ext) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = k < n_tris;
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0;
  if (in_range) { r0 = tri_verts[3 * (size_t)k]; r1 = tri_verts[3 * (size_t)k + 1]; }
  const int slot = as_i(r0.w), m = in_range ? as_i(r1.w) : -1;
  const bool mine = in_range && moved[m];
  const float* M = matrices + 16 * (size_t)(mine ? m : 0);
  v3 w[3];
  float e = 0.0f;
  if (mine) for (int j = 0; j < 3; j++) {
    const float* v = vertices + 3 * (size_t)indices[slot + j];
    w[j] = mul_m4(M, v[0], v[1], v[2], 1.0f);                                  // RS:244-246
    float a = f_abs(w[j].x); if (a < URT_INF) e = f_max(e, a);                // finite coordinates only, like the builders
    a = f_abs(w[j].y); if (a < URT_INF) e = f_max(e, a);
    a = f_abs(w[j].z); if (a < URT_INF) e = f_max(e, a);
  }
  if (mine) {
    v3 e1 = w[1] - w[0], e2 = w[2] - w[0];                                      // RS:201-202
    tri_verts[3 * (size_t)k] = make_float4(w[0].x, w[0].y, w[0].z, r0.w);
    tri_verts[3 * (size_t)k + 1] = make_float4(e1.x, e1.y, e1.z, r1.w);
    tri_verts[3 * (size_t)k + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
  }
  // largest |coordinate| per MeshObject (non-negative floats order like their bit patterns).  Leaf-order neighbours nearly always
  // belong to one MeshObject: one atomic per wave then (a million same-address atomics would serialise for ~10 ms)
  unsigned int eb = __float_as_uint(e);
  const int m0 = __shfl(m, 0, 64);
  if (__ballot(m != m0) == 0) {
    for (int off = 32; off > 0; off >>= 1) eb = max(eb, (unsigned int)__shfl_xor((int)eb, off, 64));
    if ((threadIdx.x & 63) == 0 && m0 >= 0 && moved[m0]) atomicMax(&ext[m0], eb);
  } else if (mine) atomicMax(&ext[m], eb);
}

struct Box { float lo[3], hi[3]; };

__device__ __forceinline__ Box leaf_box(const float4* __restrict__ tri_verts, int32_t code) {
  uint32_t c = ~(uint32_t)code;
  uint32_t first = c >> 3, cnt = (c & 7u) + 1u;
  Box b;
  for (int k = 0; k < 3; k++) { b.lo[k] = URT_INF; b.hi[k] = -URT_INF; }
  for (uint32_t t = 0; t < cnt; t++) {
    float4 r0 = tri_verts[3 * (size_t)(first + t)], r1 = tri_verts[3 * (size_t)(first + t) + 1], r2 = tri_verts[3 * (size_t)(first + t) + 2];
    const float p[3][3] = {{r0.x, r0.y, r0.z}, {r0.x + r1.x, r0.y + r1.y, r0.z + r1.z}, {r0.x + r2.x, r0.y + r2.y, r0.z + r2.z}};
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) { b.lo[k] = f_min(b.lo[k], p[j][k]); b.hi[k] = f_max(b.hi[k], p[j][k]); }
  }
  return b;
}

// depth of every node below its root (roots 0): the refit sweeps the levels bottom-up, one launch per level
__global__ __launch_bounds__(256) void k_depth(int n_nodes, const int32_t* __restrict__ parent, int32_t* __restrict__ depth) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  int d = 0;
  for (int p = parent[n]; p >= 0; p = parent[p]) d++;
  depth[n] = d;
}

// One level of the bottom-up refit.  cbox: per node 4 float4 = {child0.lo, child0.hi, child1.lo, child1.hi}, UNPADDED (the pad is added
// where a box is written into a node, as blas_builder.cpp does: a box is the union of its triangles, never of padded boxes).  A leaf
// child's box comes from its triangle records, an interior child's from the cbox entries the level below has just written.
__global__ __launch_bounds__(256) void k_refit_level(float4* __restrict__ nodes, int n_nodes, const float4* __restrict__ tri_verts,
                                                     const int32_t* __restrict__ depth, int level, const int32_t* __restrict__ node_mesh,
                                                     const int32_t* __restrict__ moved, const unsigned int* __restrict__ ext, float4* cbox) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes || depth[n] != level) return;
  const int m = node_mesh[n];
  if (m < 0 || !moved[m]) return;
  const float pad = __uint_as_float(ext[m]) * 1.52587890625e-5f + 1e-30f;       // blas_builder.cpp: 2^-16 x largest |coordinate| of the MeshObject
  float4 q3 = nodes[4 * (size_t)n + 3];
  const int c[2] = {as_i(q3.x), as_i(q3.y)};
  float4 lo[2], hi[2];
  for (int k = 0; k < 2; k++) {
    if (c[k] < 0) {
      Box b = leaf_box(tri_verts, c[k]);
      lo[k] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.0f); hi[k] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
    } else {
      float4 l0 = cbox[4 * (size_t)c[k]], h0 = cbox[4 * (size_t)c[k] + 1], l1 = cbox[4 * (size_t)c[k] + 2], h1 = cbox[4 * (size_t)c[k] + 3];
      lo[k] = make_float4(f_min(l0.x, l1.x), f_min(l0.y, l1.y), f_min(l0.z, l1.z), 0.0f);
      hi[k] = make_float4(f_max(h0.x, h1.x), f_max(h0.y, h1.y), f_max(h0.z, h1.z), 0.0f);
    }
    cbox[4 * (size_t)n + 2 * k] = lo[k];
    cbox[4 * (size_t)n + 2 * k + 1] = hi[k];
  }
  nodes[4 * (size_t)n] = make_float4(lo[0].x - pad, lo[0].y - pad, lo[0].z - pad, hi[0].x + pad);
  nodes[4 * (size_t)n + 1] = make_float4(hi[0].y + pad, hi[0].z + pad, lo[1].x - pad, lo[1].y - pad);
  nodes[4 * (size_t)n + 2] = make_float4(lo[1].z - pad, hi[1].x + pad, hi[1].y + pad, hi[1].z + pad);
}

// The shading normals of the leaf-order triangles of every MeshObject with flagged[m] != 0, from the device copy of _Normals: the slot of a
// triangle's first index is kept in its record (v0.w), its MeshObject in e1.w, as k_refit_tris reads them.
__global__ __launch_bounds__(256) void k_refit_norms(float4* __restrict__ tri_norms, const float4* __restrict__ tri_verts, int n_tris,
                                                     const float* __restrict__ normals, const int32_t* __restrict__ indices,
                                                     const int32_t* __restrict__ flagged) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_tris) return;
  const int slot = as_i(tri_verts[3 * (size_t)k].w), m = as_i(tri_verts[3 * (size_t)k + 1].w);
  if (!flagged[m]) return;
  for (int j = 0; j < 3; j++) {
    const float* p = normals + 3 * (size_t)indices[slot + j];                   // RS:259-261
    tri_norms[3 * (size_t)k + j] = make_float4(p[0], p[1], p[2], 0.0f);
  }
}

__device__ __forceinline__ double box_area(float lx, float ly, float lz, float hx, float hy, float hz) {
  const double dx = (double)hx - (double)lx, dy = (double)hy - (double)ly, dz = (double)hz - (double)lz;
  return 2.0 * (dx * dy + dy * dz + dz * dx);
}

// Surface-area cost: every node adds area(child box) x (triangles of a leaf child, 1 for an interior child) for both children to its
// MeshObject's sum out[2 m]; a root also writes the area of the union of its two child boxes to out[2 m + 1] (the host divides).  Terms that
// are not finite add nothing.  The sums are float64 and added with the hardware's float64 atomic (`out` is the library's own device memory).
// Same-address atomics are what bounds this kernel (one per wave: 6 - 15 ns each), so they are made few: a wave reduces the terms of its
// first pending lane's MeshObject, then of the next one's, until none is left — neighbouring nodes nearly always belong to one MeshObject,
// whichever builder numbered them — and the first such sum of each of a workgroup's four waves is combined in LDS before it is added.
__global__ __launch_bounds__(256) void k_tree_cost(const float4* __restrict__ nodes, int n_nodes, const int32_t* __restrict__ parent,
                                                   const int32_t* __restrict__ node_mesh, int n_meshes, double* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  int m = n < n_nodes ? node_mesh[n] : -1;
  if (m >= n_meshes) m = -1;
  double t = 0.0;
  if (m >= 0) {
    const float4 q0 = nodes[4 * (size_t)n], q1 = nodes[4 * (size_t)n + 1], q2 = nodes[4 * (size_t)n + 2], q3 = nodes[4 * (size_t)n + 3];
    const int c0 = as_i(q3.x), c1 = as_i(q3.y);
    const double a0 = box_area(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y) * (c0 < 0 ? (double)(((~(uint32_t)c0) & 7u) + 1u) : 1.0);
    const double a1 = box_area(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w) * (c1 < 0 ? (double)(((~(uint32_t)c1) & 7u) + 1u) : 1.0);
    if (a0 - a0 == 0.0) t += a0;                                                  // finite
    if (a1 - a1 == 0.0) t += a1;
    if (parent[n] < 0)
      out[2 * (size_t)m + 1] = box_area(f_min(q0.x, q1.z), f_min(q0.y, q1.w), f_min(q0.z, q2.x), f_max(q0.w, q2.y), f_max(q1.x, q2.z), f_max(q1.y, q2.w));
  }
  __shared__ int s_mesh[4];
  __shared__ double s_sum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_mesh[wave] = -1; s_sum[wave] = 0.0; }
  unsigned long long pending = __ballot(m >= 0 && t != 0.0);
  for (bool first = true; pending; first = false) {
    const int leader = __ffsll((long long)pending) - 1;
    const int ml = __shfl(m, leader, 64);
    double v = m == ml ? t : 0.0;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == leader) {
      if (first) { s_mesh[wave] = ml; s_sum[wave] = v; }
      else unsafeAtomicAdd(&out[2 * (size_t)ml], v);
    }
    pending &= ~__ballot(m == ml);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int cm = -1;
    double cv = 0.0;
    for (int w = 0; w < 4; w++) {
      if (s_mesh[w] < 0) continue;
      if (s_mesh[w] != cm) {
        if (cm >= 0) unsafeAtomicAdd(&out[2 * (size_t)cm], cv);
        cm = s_mesh[w]; cv = 0.0;
      }
      cv += s_sum[w];
    }
    if (cm >= 0) unsafeAtomicAdd(&out[2 * (size_t)cm], cv);
  }
}

}  // namespace

namespace urtd {

hipError_t refit_norms(float4* tri_norms, const float4* tri_verts, int n_tris, const float* normals, const int32_t* indices,
                       const int32_t* flagged, hipStream_t st) {
  if (n_tris <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_refit_norms, dim3((n_tris + 255) / 256), dim3(256), 0, st, tri_norms, tri_verts, n_tris, normals, indices, flagged);
  return hipGetLastError();
}

hipError_t tree_cost(const float4* nodes, int n_nodes, const int32_t* parent, const int32_t* node_mesh, int n_meshes, double* out, hipStream_t st) {
  if (n_meshes <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(double) * (size_t)n_meshes, st);
  if (e != hipSuccess || n_nodes <= 0) return e;
  hipLaunchKernelGGL(k_tree_cost, dim3((n_nodes + 255) / 256), dim3(256), 0, st, nodes, n_nodes, parent, node_mesh, n_meshes, out);
  return hipGetLastError();
}

hipError_t refit_prepare(const float4* nodes, int n_nodes, const float4* tri_verts, int32_t* parent, int32_t* node_mesh, int32_t* depth, hipStream_t st) {
  if (n_nodes <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(parent, 0xff, sizeof(int32_t) * (size_t)n_nodes, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(node_mesh, 0xff, sizeof(int32_t) * (size_t)n_nodes, st);
  if (e != hipSuccess) return e;
  int nb = (n_nodes + 255) / 256;
  hipLaunchKernelGGL(k_parents, dim3(nb), dim3(256), 0, st, nodes, n_nodes, parent);
  hipLaunchKernelGGL(k_node_mesh, dim3(nb), dim3(256), 0, st, nodes, tri_verts, n_nodes, (const int32_t*)parent, node_mesh);
  hipLaunchKernelGGL(k_depth, dim3(nb), dim3(256), 0, st, n_nodes, (const int32_t*)parent, depth);
  return hipGetLastError();
}

hipError_t refit_moved(float4* nodes, int n_nodes, float4* tri_verts, int n_tris, const float* vertices, const int32_t* indices,
                       const int32_t* depth, int max_level, const int32_t* node_mesh, const float* matrices, const int32_t* moved,
                       unsigned int* ext, int n_meshes, float4* cbox, hipStream_t st) {
  if (n_tris <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(ext, 0, sizeof(unsigned int) * (size_t)n_meshes, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_refit_tris, dim3((n_tris + 255) / 256), dim3(256), 0, st, tri_verts, n_tris, vertices, indices, matrices, moved, ext);
  for (int level = max_level; level >= 0 && n_nodes > 0; level--)               // bottom-up: a level reads what the level below wrote (stream order)
    hipLaunchKernelGGL(k_refit_level, dim3((n_nodes + 255) / 256), dim3(256), 0, st, nodes, n_nodes, (const float4*)tri_verts, depth, level, node_mesh,
                       moved, (const unsigned int*)ext, cbox);
  return hipGetLastError();
}

}  // namespace urtd
