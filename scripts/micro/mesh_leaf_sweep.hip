// mesh_leaf_sweep.hip — how B (csrc/object_bvh.h kMeshLeafBlocks, the per-MeshObject workgroup cap of urt_mesh_leaf_bounds_device) was
// chosen: the two kernels of csrc/object_bvh.hip, compiled with another B, timed on MeshObject sizes like the benchmark scenes'.
//   for B in 16 64 256 1024; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DURT_EXPERIMENT -DURT_MESH_LEAF_BLOCKS_SWEEP=$B \
//     scripts/micro/mesh_leaf_sweep.hip -o scripts/micro/mesh_leaf_sweep_$B; done
// Prints, per scene, the median and the range of 9 timings (device events around 20 calls each) in microseconds per call.
#include "../../unityraytracer_amd/csrc/object_bvh.hip"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

struct Scene { const char* name; std::vector<int> tris; };

int main() {
  const Scene scenes[] = {
      {"C3-like: one mesh of 69,600 triangles", {69600}},
      {"C4-like: three meshes of 98,304 triangles, six of 852", {98304, 98304, 98304, 852, 852, 852, 852, 852, 852}},
      {"C5-like: twelve meshes of 81,920 triangles", std::vector<int>(12, 81920)},
      {"one mesh of 4,000,000 triangles", {4000000}},
  };
  std::mt19937 rng(7);
  for (const Scene& sc : scenes) {
    const int n = (int)sc.tris.size();
    std::vector<float> mo((size_t)n * 28, 0.0f);
    std::vector<int32_t> idx;
    std::vector<float> verts;
    for (int m = 0; m < n; m++) {
      const int slots = 3 * sc.tris[m], nv = sc.tris[m] / 2 + 2, v0 = (int)(verts.size() / 3);
      float* rec = mo.data() + (size_t)m * 28;
      rec[0] = rec[5] = rec[10] = rec[15] = 1.0f; rec[12] = (float)m;
      const int32_t off = (int32_t)idx.size();
      std::memcpy(rec + 16, &off, 4); std::memcpy(rec + 17, &slots, 4);
      std::uniform_real_distribution<float> pos(-1.0f, 1.0f);
      for (int i = 0; i < 3 * nv; i++) verts.push_back(pos(rng));
      // a triangle names vertices near each other, as an indexed mesh does
      std::uniform_int_distribution<int> near(0, 63);
      for (int t = 0; t < sc.tris[m]; t++) for (int c = 0; c < 3; c++) idx.push_back(v0 + std::min(nv - 1, t / 2 + near(rng)));
    }
    char *d_mo, *d_leaves; float *d_v, *d_partial; int32_t* d_idx;
    CHECK(hipMalloc(&d_mo, mo.size() * 4)); CHECK(hipMalloc(&d_v, verts.size() * 4)); CHECK(hipMalloc(&d_idx, idx.size() * 4));
    CHECK(hipMalloc(&d_partial, (size_t)n * urtd::kMeshLeafBlocks * urtd::kMeshLeafWords * 4)); CHECK(hipMalloc(&d_leaves, (size_t)n * 28));
    CHECK(hipMemcpy(d_mo, mo.data(), mo.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_v, verts.data(), verts.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    auto call = [&]() { return urtd::mesh_leaf_bounds(d_mo, n, d_v, (int)(verts.size() / 3), d_idx, (int)idx.size(), d_partial, d_leaves, nullptr); };
    for (int i = 0; i < 5; i++) CHECK(call());
    CHECK(hipDeviceSynchronize());
    std::vector<float> us;
    for (int rep = 0; rep < 9; rep++) {
      CHECK(hipEventRecord(e0, nullptr));
      for (int i = 0; i < 20; i++) CHECK(call());
      CHECK(hipEventRecord(e1, nullptr));
      CHECK(hipEventSynchronize(e1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      us.push_back(ms * 1000.0f / 20.0f);
    }
    std::sort(us.begin(), us.end());
    std::printf("B %4d  %-58s median %8.2f us per call [%.2f .. %.2f]\n", urtd::kMeshLeafBlocks, sc.name, us[4], us.front(), us.back());
    CHECK(hipFree(d_mo)); CHECK(hipFree(d_v)); CHECK(hipFree(d_idx)); CHECK(hipFree(d_partial)); CHECK(hipFree(d_leaves));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
  }
  // the heap kernel (one workgroup; it does not depend on B): random boxes
  for (int n : {12, 64, 256, 1024}) {
    int depth = 1;
    while ((1 << (depth - 1)) < n) depth++;
    const int len = (1 << depth) - 1;
    std::vector<float> leaves((size_t)n * 7);
    std::uniform_real_distribution<float> pos(-10.0f, 10.0f);
    for (int i = 0; i < n; i++) {
      for (int k = 0; k < 3; k++) { leaves[7 * i + k] = pos(rng); leaves[7 * i + 3 + k] = leaves[7 * i + k] + 1.0f; }
      std::memcpy(&leaves[7 * i + 6], &i, 4);
    }
    char *d_leaves, *d_nodes;
    CHECK(hipMalloc(&d_leaves, (size_t)n * 28)); CHECK(hipMalloc(&d_nodes, (size_t)len * 28));
    CHECK(hipMemcpy(d_leaves, leaves.data(), (size_t)n * 28, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 5; i++) CHECK(urtd::build_object_bvh(d_leaves, n, d_nodes, len, nullptr));
    CHECK(hipDeviceSynchronize());
    std::vector<float> us;
    for (int rep = 0; rep < 9; rep++) {
      CHECK(hipEventRecord(e0, nullptr));
      for (int i = 0; i < 20; i++) CHECK(urtd::build_object_bvh(d_leaves, n, d_nodes, len, nullptr));
      CHECK(hipEventRecord(e1, nullptr));
      CHECK(hipEventSynchronize(e1));
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      us.push_back(ms * 1000.0f / 20.0f);
    }
    std::sort(us.begin(), us.end());
    std::printf("heap of %4d leaves (%4d nodes)  median %8.2f us per call [%.2f .. %.2f]\n", n, len, us[4], us.front(), us.back());
    CHECK(hipFree(d_leaves)); CHECK(hipFree(d_nodes));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
  }
  return 0;
}
