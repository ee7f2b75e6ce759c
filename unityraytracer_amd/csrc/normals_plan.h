// normals_plan.h — the weld relation of RayTraceMaster.ComputeNormals (RM:340-368) and the plan a GPU pass over it needs
// (csrc/normals_plan.cpp).  Pure C++: no HIP, no include/urt.h, so that the file also builds on its own under a host sanitizer
// (tests/normals_plan_main.cpp).  Private.
//
// The reference gives vertex i the sum, in ascending slot order, of the un-normalised face normals of every index slot j whose vertex
// satisfies (v_i - v_indices[j]).sqrMagnitude <= EPSILON = 3 * float.Epsilon.  That is plain equality (-0 == +0) except for
// differences so small that their squares underflow: two DIFFERENT positions can only pass when, on every axis, their coordinates are
// equal or both of magnitude below 2^-50 (distinct floats of magnitude >= 2^-50 differ by >= 2^-73, whose square 1.1e-44 already
// exceeds EPSILON; numerical zeros like sin(pi) * r = 1e-17 are common in real meshes, so this is not a corner to ignore).  Such
// PARTNER groups are found pair by pair with the reference's own float test: the relation is not transitive.
#pragma once
#include <cstdint>
#include <vector>

namespace urtd {

// Vertices grouped by exact position, and which groups weld with OTHER groups.
struct NormalsGroups {
  std::vector<int> group_of;                  // vertex -> group, numbered in the order of first appearance
  std::vector<int> rep;                       // group -> its first vertex
  std::vector<int> partner_slot;              // group -> index into `partners`, or -1 (the common case)
  std::vector<std::vector<int>> partners;     // the groups a group welds with, itself excluded
};
void normals_groups(const float* vertices, int n_vertices, NormalsGroups& out);

// The canonical plan for the served vertices first .. first + count - 1 (include/urt.h, "Normals on the device").
struct NormalsPlan {
  int first = 0, count = 0;
  std::vector<int32_t> tris;                  // 3 vertex indices per needed triangle, ascending original triangle number
  std::vector<int32_t> entries;               // compact triangle ids (positions in `tris`), one per contributing slot, ascending slot order per list
  std::vector<int32_t> ranges;                // {start, length} into `entries` per served vertex
  int n_lists = 0, max_valence = 0;
};
enum { kNormalsPlanOk = 0, kNormalsPlanBadIndex = 1 };
// n_indices is a multiple of 3 and the served range lies inside the vertices (the callers check); every index slot of `indices` takes
// part in the weld.  kNormalsPlanBadIndex: an index outside the vertices (out is unspecified then).  Allocation failures throw.
int normals_plan_build(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int first, int count, NormalsPlan& out);

}  // namespace urtd
