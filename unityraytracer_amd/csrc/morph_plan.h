// morph_plan.h — the plan of include/urt.h urt_morph_vertices ("blend shapes on the device"): the deltas of every blend-shape target
// laid out per served vertex (CSR by vertex), which is what one lane of csrc/morph.hip walks (csrc/morph_plan.cpp).  Pure C++: no HIP,
// no include/urt.h, so that the file also builds on its own under a host sanitizer (tests/morph_plan_main.cpp).  Private.
#pragma once
#include <cstdint>
#include <vector>

namespace urtd {

// urt_MorphDelta of include/urt.h, member for member (geometry_ops.cpp asserts the size).
struct MorphDeltaIn {
  int32_t vertex, target;
  float dp[3], dn[3];
};

// The canonical plan for the served vertices first .. first + count - 1: `order` holds the input delta numbers sorted by vertex, then by
// target, then by input position (duplicates of one (vertex, target) pair are kept); nothing is pruned.
struct MorphPlan {
  int first = 0, count = 0, n_targets = 0;
  std::vector<int32_t> order;                 // n_deltas input positions
  std::vector<int32_t> ranges;                // {start, length} into `order` per served vertex
  int max_valence = 0, n_touched = 0;         // the longest list; the served vertices whose list is not empty
};
enum { kMorphPlanOk = 0, kMorphPlanBadVertex = 1, kMorphPlanBadTarget = 2 };
constexpr int kMorphMaxTargets = 4096;        // a weight table of at most 16 KB
// n_deltas >= 0, first >= 0, count >= 0 and 1 <= n_targets <= kMorphMaxTargets (the callers check).  kMorphPlanBadVertex: a delta names
// a vertex outside the served range; kMorphPlanBadTarget: a target outside 0 .. n_targets - 1 (out is unspecified then).  Allocation
// failures throw.
int morph_plan_build(const MorphDeltaIn* deltas, int n_deltas, int n_targets, int first, int count, MorphPlan& out);

}  // namespace urtd
