// normals_plan_main.cpp — a stand-alone program over csrc/normals_plan.cpp for a host sanitizer build (tests/test_normals_abi.py
// compiles both with g++ -fsanitize=address,undefined and runs the result): plans for small meshes written out as arrays, for
// sub-spans of them and for an out-of-range index.  Exit status 0: every plan kept its invariants and the sanitizers saw nothing.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../unityraytracer_amd/csrc/normals_plan.h"

using urtd::NormalsPlan;

namespace {

int g_failures = 0;
#define EXPECT(cond, what)                                                        \
  do {                                                                            \
    if (!(cond)) { std::printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__); g_failures++; } \
  } while (0)

// what every plan must hold, whatever the mesh
void check_invariants(const char* what, const NormalsPlan& p, int n_vertices, int n_indices) {
  const int nt = (int)p.tris.size() / 3, ne = (int)p.entries.size();
  EXPECT((int)p.ranges.size() == 2 * p.count, what);
  EXPECT(nt <= n_indices / 3, what);
  for (int32_t i : p.tris) EXPECT(i >= 0 && i < n_vertices, what);
  for (int32_t e : p.entries) EXPECT(e >= 0 && e < nt, what);
  int longest = 0;
  for (int k = 0; k < p.count; k++) {
    const int start = p.ranges[2 * (size_t)k], len = p.ranges[2 * (size_t)k + 1];
    EXPECT(start >= 0 && len >= 0 && start + len <= ne, what);
    longest = len > longest ? len : longest;
  }
  EXPECT(longest == p.max_valence, what);
  std::vector<char> used((size_t)nt, 0);
  for (int32_t e : p.entries) if (e >= 0 && e < nt) used[(size_t)e] = 1;
  for (char u : used) EXPECT(u, what);                      // only needed triangles are kept
}

NormalsPlan build(const char* what, const std::vector<float>& v, const std::vector<int32_t>& t, int first, int count, int expect = urtd::kNormalsPlanOk) {
  NormalsPlan p;
  const int rc = urtd::normals_plan_build(v.data(), (int)v.size() / 3, t.data(), (int)t.size(), first, count, p);
  EXPECT(rc == expect, what);
  if (rc == urtd::kNormalsPlanOk) check_invariants(what, p, (int)v.size() / 3, (int)t.size());
  return p;
}

int length_of(const NormalsPlan& p, int vertex) { return p.ranges[2 * (size_t)(vertex - p.first) + 1]; }

}  // namespace

int main() {
  // a cube of 24 vertices, four per face: every corner welded three ways
  std::vector<float> cube;
  std::vector<int32_t> cube_t;
  for (int axis = 0; axis < 3; axis++)
    for (int side = 0; side < 2; side++) {
      const int u = (axis + 1) % 3, w = (axis + 2) % 3, base = (int)cube.size() / 3;
      const int du[4] = {-1, 1, 1, -1}, dw[4] = {-1, -1, 1, 1};
      for (int k = 0; k < 4; k++) {
        float p[3];
        p[axis] = side ? 1.0f : -1.0f; p[u] = (float)du[k]; p[w] = (float)dw[k];
        cube.insert(cube.end(), p, p + 3);
      }
      const int quad[6] = {base, base + 1, base + 2, base, base + 2, base + 3};
      for (int k = 0; k < 6; k++) cube_t.push_back(quad[side ? k : 5 - k]);
    }
  {
    NormalsPlan p = build("cube", cube, cube_t, 0, 24);
    EXPECT(p.n_lists == 8 && p.tris.size() == 36 && p.entries.size() == 36, "cube");
    NormalsPlan q = build("cube, one face", cube, cube_t, 4, 4);
    EXPECT(q.n_lists == 4, "cube, one face");
    build("cube, nothing served", cube, cube_t, 24, 0);
  }
  // two quads that share an edge, as two MeshObjects hold them
  const std::vector<float> quads = {0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 2, 0.5f, 0, 2, 0.5f, 1, 1, 0, 1};
  const std::vector<int32_t> quads_t = {0, 2, 1, 0, 3, 2, 4, 6, 5, 4, 7, 6};
  {
    NormalsPlan p = build("two quads, the first", quads, quads_t, 0, 4);
    EXPECT(p.tris.size() == 12, "two quads, the first");      // the neighbour's triangles are needed along the shared edge
    EXPECT(length_of(p, 1) == 3 && length_of(p, 2) == 3 && length_of(p, 0) == 2 && length_of(p, 3) == 1, "two quads, the first");
  }
  // a fan, a collinear triangle, a vertex no triangle names, a triangle with two slots on welded vertices
  const std::vector<float> odd = {0, 0, 0, 1, 0, 0, 0, 0, 1, -1, 0.3f, 0, 5, 5, 5, 6, 6, 6, 7, 7, 7, 9, 9, 9, 3, 0, 0, 3, 0, 0, 3, 1, 0, 4, 0, 1};
  const std::vector<int32_t> odd_t = {0, 2, 1, 0, 3, 2, 4, 5, 6, 8, 9, 10, 8, 11, 10, 9, 10, 11};
  {
    NormalsPlan p = build("odd ones", odd, odd_t, 0, 12);
    EXPECT(length_of(p, 7) == 0 && length_of(p, 8) == 4 && length_of(p, 9) == 4, "odd ones");
    EXPECT(p.ranges[16] == p.ranges[18], "odd ones");         // welded duplicates share one list
    build("odd ones, the unreferenced vertex alone", odd, odd_t, 7, 1);
  }
  // the partner rule: equal (-0), a partner (1e-30), no partner (1e-17), and a trio that is not transitive
  std::vector<float> tiny = {0, 0, 0, 1e-17f, 0, 0, -0.0f, 0, -0.0f, 1e-30f, 0, 0, 0, 2, 0, 5e-23f, 2, 0, 1e-22f, 2, 0};
  std::vector<int32_t> tiny_t;
  for (int k = 0; k < 7; k++) {
    const int b = (int)tiny.size() / 3;
    const float far[6] = {1.0f + 0.25f * k, 0.5f * k, 0.125f * k, 0.25f * k - 0.5f, 1.0f + k, 1.0f + 0.5f * k};
    tiny.insert(tiny.end(), far, far + 6);
    tiny_t.insert(tiny_t.end(), {k, b, b + 1});
  }
  {
    NormalsPlan p = build("partners", tiny, tiny_t, 0, (int)tiny.size() / 3);
    const int want[7] = {3, 1, 3, 3, 2, 3, 2};
    for (int k = 0; k < 7; k++) EXPECT(length_of(p, k) == want[k], "partners");
    build("partners, a sub-span", tiny, tiny_t, 3, 3);
  }
  // positions that are not finite flow through the grouping
  {
    std::vector<float> bad = quads;
    bad[3] = NAN; bad[12] = NAN; bad[7] = INFINITY; bad[22] = -INFINITY;
    build("non-finite positions", bad, quads_t, 0, 8);
  }
  // an index outside the vertices, on either side, and no triangles at all
  {
    std::vector<int32_t> t = quads_t;
    t[7] = 8;
    build("index too large", quads, t, 0, 8, urtd::kNormalsPlanBadIndex);
    t[7] = -1;
    build("index negative", quads, t, 0, 8, urtd::kNormalsPlanBadIndex);
    NormalsPlan p = build("no triangles", quads, std::vector<int32_t>(), 0, 8);
    EXPECT(p.n_lists == 6 && p.entries.empty() && p.tris.empty() && p.max_valence == 0, "no triangles");
    build("nothing at all", std::vector<float>(), std::vector<int32_t>(), 0, 0);
  }
  // the grouping alone, as urt_host_compute_normals uses it
  {
    urtd::NormalsGroups G;
    urtd::normals_groups(tiny.data(), (int)tiny.size() / 3, G);
    EXPECT(G.group_of[0] == G.group_of[2] && G.group_of[0] != G.group_of[3], "groups");
    EXPECT(G.partner_slot[(size_t)G.group_of[1]] < 0 && G.partner_slot[(size_t)G.group_of[5]] >= 0, "groups");
    EXPECT(G.partners[(size_t)G.partner_slot[(size_t)G.group_of[5]]].size() == 2, "groups");
  }
  if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
  std::printf("normals plans: ok\n");
  return 0;
}
