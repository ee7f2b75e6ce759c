// normals_plan.cpp — see normals_plan.h.  The grouping is what urt_host_compute_normals (host_scene.cpp) sums over; the plan lays the
// same relation out for csrc/normals.hip: one list of contributing triangles per served vertex, in ascending slot order.
#include "normals_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

namespace urtd {
namespace {

struct Key {
  uint32_t a, b, c;
  bool operator==(const Key& o) const { return a == o.a && b == o.b && c == o.c; }
};
struct KeyHash {
  size_t operator()(const Key& k) const {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ k.a;
    h = (h ^ (h >> 32)) * 0xBF58476D1CE4E5B9ull + k.b;
    h = (h ^ (h >> 29)) * 0x94D049BB133111EBull + k.c;
    return (size_t)(h ^ (h >> 31));
  }
};
inline uint32_t bits_no_negzero(float f) {           // -0 == +0 for the reference's (a - b).sqrMagnitude test
  uint32_t u; std::memcpy(&u, &f, 4);
  return u == 0x80000000u ? 0u : u;
}

}  // namespace

void normals_groups(const float* vertices, int n_vertices, NormalsGroups& out) {
  // Step 1: exact groups (O(V) position hash).
  std::unordered_map<Key, int, KeyHash> groups;
  groups.reserve((size_t)n_vertices * 2);
  out.group_of.assign((size_t)n_vertices, 0);
  out.rep.clear();
  for (int i = 0; i < n_vertices; i++) {
    Key k{bits_no_negzero(vertices[3 * (size_t)i]), bits_no_negzero(vertices[3 * (size_t)i + 1]), bits_no_negzero(vertices[3 * (size_t)i + 2])};
    auto it = groups.find(k);
    if (it == groups.end()) { it = groups.emplace(k, (int)groups.size()).first; out.rep.push_back(i); }
    out.group_of[(size_t)i] = it->second;
  }
  const size_t ng = groups.size();
  // Step 2: groups that weld with OTHER groups.  Candidates share a coarse key (coordinates below 2^-50 mapped to 0);
  // inside a coarse bucket the reference's float test decides, pair by pair (the relation is not transitive).
  const float kTiny = 8.8817842e-16f;                     // 2^-50
  const float kEps = 3.0f * 1.401298464e-45f;              // RM:14
  out.partners.clear();
  out.partner_slot.assign(ng, -1);
  std::unordered_map<Key, std::vector<int>, KeyHash> coarse;
  for (size_t g = 0; g < ng; g++) {
    const float* p = vertices + 3 * (size_t)out.rep[g];
    bool has_small = false;
    uint32_t kk[3];
    for (int c = 0; c < 3; c++) { bool small = std::fabs(p[c]) < kTiny; has_small = has_small || small; kk[c] = small ? 0u : bits_no_negzero(p[c]); }
    if (has_small) coarse[Key{kk[0], kk[1], kk[2]}].push_back((int)g);
  }
  for (auto& kv : coarse) {
    const std::vector<int>& b = kv.second;
    if (b.size() < 2) continue;
    for (size_t x = 0; x < b.size(); x++)
      for (size_t y = x + 1; y < b.size(); y++) {
        const float* p = vertices + 3 * (size_t)out.rep[(size_t)b[x]];
        const float* q = vertices + 3 * (size_t)out.rep[(size_t)b[y]];
        const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
        if (dx * dx + dy * dy + dz * dz <= kEps) {
          for (int side = 0; side < 2; side++) {
            int g = side ? b[y] : b[x], o = side ? b[x] : b[y];
            if (out.partner_slot[(size_t)g] < 0) { out.partner_slot[(size_t)g] = (int)out.partners.size(); out.partners.emplace_back(); }
            out.partners[(size_t)out.partner_slot[(size_t)g]].push_back(o);
          }
        }
      }
  }
}

int normals_plan_build(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int first, int count, NormalsPlan& out) {
  out = NormalsPlan();
  out.first = first; out.count = count;
  for (int j = 0; j < n_indices; j++)
    if (indices[j] < 0 || indices[j] >= n_vertices) return kNormalsPlanBadIndex;
  out.ranges.assign(2 * (size_t)count, 0);
  if (count == 0) return kNormalsPlanOk;
  NormalsGroups G;
  normals_groups(vertices, n_vertices, G);
  const size_t ng = G.rep.size();
  // the groups whose own slots are needed: those of the served vertices and their partners
  std::vector<char> collect(ng, 0);
  for (int v = first; v < first + count; v++) {
    const int g = G.group_of[(size_t)v];
    collect[(size_t)g] = 1;
    if (G.partner_slot[(size_t)g] >= 0) for (int o : G.partners[(size_t)G.partner_slot[(size_t)g]]) collect[(size_t)o] = 1;
  }
  // their own slots, ascending (counting sort over the index slots)
  std::vector<int> own_start(ng + 1, 0);
  for (int j = 0; j < n_indices; j++) { const int g = G.group_of[(size_t)indices[j]]; if (collect[(size_t)g]) own_start[(size_t)g + 1]++; }
  for (size_t g = 0; g < ng; g++) own_start[g + 1] += own_start[g];
  std::vector<int> own((size_t)own_start[ng]), fill(own_start.begin(), own_start.end() - 1);
  for (int j = 0; j < n_indices; j++) { const int g = G.group_of[(size_t)indices[j]]; if (collect[(size_t)g]) own[(size_t)fill[(size_t)g]++] = j; }
  // the lists, in the order of the first served vertex that uses them: slots first, compact triangle ids below
  std::vector<int> list_start(ng, -1), list_len(ng, 0), slots, merged;
  for (int v = first; v < first + count; v++) {
    const size_t g = (size_t)G.group_of[(size_t)v];
    if (list_start[g] < 0) {
      list_start[g] = (int)slots.size();
      const int ps = G.partner_slot[g];
      if (ps < 0) slots.insert(slots.end(), own.begin() + own_start[g], own.begin() + own_start[g + 1]);
      else {                                                // the union with the partners' slots, in ascending slot order
        merged.assign(own.begin() + own_start[g], own.begin() + own_start[g + 1]);
        for (int o : G.partners[(size_t)ps]) merged.insert(merged.end(), own.begin() + own_start[(size_t)o], own.begin() + own_start[(size_t)o + 1]);
        std::sort(merged.begin(), merged.end());
        slots.insert(slots.end(), merged.begin(), merged.end());
      }
      list_len[g] = (int)slots.size() - list_start[g];
      out.n_lists++;
      out.max_valence = std::max(out.max_valence, list_len[g]);
    }
    out.ranges[2 * (size_t)(v - first)] = list_start[g];
    out.ranges[2 * (size_t)(v - first) + 1] = list_len[g];
  }
  // the needed triangles, ascending, and their compact ids
  std::vector<int32_t> compact((size_t)n_indices / 3, -1);
  for (int j : slots) compact[(size_t)j / 3] = 0;
  int32_t nt = 0;
  for (size_t t = 0; t < compact.size(); t++) if (compact[t] == 0) compact[t] = nt++;
  out.tris.resize(3 * (size_t)nt);
  for (size_t t = 0; t < compact.size(); t++)
    if (compact[t] >= 0) for (int c = 0; c < 3; c++) out.tris[3 * (size_t)compact[t] + (size_t)c] = indices[3 * t + (size_t)c];
  out.entries.resize(slots.size());
  for (size_t k = 0; k < slots.size(); k++) out.entries[k] = compact[(size_t)slots[k] / 3];
  return kNormalsPlanOk;
}

}  // namespace urtd
