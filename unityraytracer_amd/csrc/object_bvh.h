// object_bvh.h — the object-level BVH on the device (csrc/object_bvh.hip): the leaf boxes of _MeshObjects and _Spheres and the implicit
// heap over them, written into buffer mirrors.  What include/urt.h says of urt_mesh_leaf_bounds_device, urt_sphere_leaf_bounds_device
// and urt_build_object_bvh_device is normative.  Private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace urtd {

#ifndef URT_MESH_LEAF_BLOCKS_SWEEP
constexpr int kMeshLeafBlocks = 256;         // B: at most this many workgroups (of 256 index slots per pass) work on one MeshObject
#else
constexpr int kMeshLeafBlocks = URT_MESH_LEAF_BLOCKS_SWEEP;   // scripts/micro/mesh_leaf_sweep.hip: how B was chosen
#endif
constexpr int kMeshLeafWords = 8;            // one partial: min.xyz, max.xyz, the count (as bits), 0
constexpr int kObjectBvhDeviceMax = 1024;    // URT_OBJECT_BVH_DEVICE_MAX: the heap kernel is ONE workgroup, one lane per leaf

// mesh_objects: n_meshes records of 112 bytes; partial holds n_meshes * kMeshLeafBlocks * kMeshLeafWords floats; leaves n_meshes records
// of 28 bytes.  n_meshes > 0.
hipError_t mesh_leaf_bounds(const char* mesh_objects, int n_meshes, const float* vertices, int n_vertices, const int32_t* indices,
                            int n_indices, float* partial, char* leaves, hipStream_t st);
// spheres: n records of 56 bytes; leaves n records of 28 bytes.  n > 0.
hipError_t sphere_leaf_bounds(const char* spheres, int n, char* leaves, hipStream_t st);
// leaves: n records of 28 bytes, 1 <= n <= kObjectBvhDeviceMax; nodes: len = urt_host_object_bvh_length(n) records of 28 bytes.
hipError_t build_object_bvh(const char* leaves, int n, char* nodes, int len, hipStream_t st);

}  // namespace urtd
