// morph_plan.cpp — see morph_plan.h.  A counting sort by vertex (stable: input order survives), then each vertex's short list is
// sorted by target, stably again, so that duplicates of one (vertex, target) pair stay in input order.
#include "morph_plan.h"

#include <algorithm>

namespace urtd {

int morph_plan_build(const MorphDeltaIn* deltas, int n_deltas, int n_targets, int first, int count, MorphPlan& out) {
  out = MorphPlan();
  out.first = first; out.count = count; out.n_targets = n_targets;
  const long long end = (long long)first + (long long)count;
  for (int k = 0; k < n_deltas; k++) {
    if ((long long)deltas[k].vertex < (long long)first || (long long)deltas[k].vertex >= end) return kMorphPlanBadVertex;
    if (deltas[k].target < 0 || deltas[k].target >= n_targets) return kMorphPlanBadTarget;
  }
  out.ranges.assign(2 * (size_t)count, 0);
  out.order.resize((size_t)n_deltas);
  if (count == 0) return kMorphPlanOk;                      // (then n_deltas is 0 as well: no vertex is served)
  for (int k = 0; k < n_deltas; k++) out.ranges[2 * (size_t)(deltas[k].vertex - first) + 1]++;
  int32_t at = 0;
  for (int v = 0; v < count; v++) {
    const int32_t len = out.ranges[2 * (size_t)v + 1];
    out.ranges[2 * (size_t)v] = at;
    at += len;
    out.max_valence = std::max(out.max_valence, (int)len);
    out.n_touched += len > 0;
  }
  std::vector<int32_t> fill((size_t)count);
  for (int v = 0; v < count; v++) fill[(size_t)v] = out.ranges[2 * (size_t)v];
  for (int k = 0; k < n_deltas; k++) out.order[(size_t)fill[(size_t)(deltas[k].vertex - first)]++] = k;
  for (int v = 0; v < count; v++) {
    const auto b = out.order.begin() + out.ranges[2 * (size_t)v];
    std::stable_sort(b, b + out.ranges[2 * (size_t)v + 1], [deltas](int32_t x, int32_t y) { return deltas[x].target < deltas[y].target; });
  }
  return kMorphPlanOk;
}

}  // namespace urtd
