// scene_prep.cpp — the device scene, derived from the bound ComputeBuffers (context_impl.h: urt_context::Scene).
// prepare_scene runs at the first dispatch / query / feature-buffer call after a change: in place when only the small tables
// and object poses changed (prepare_incremental), from scratch otherwise.
#include "experiments.h"
#include "context_impl.h"

#include <chrono>

#include "lbvh.h"
#include "index_span.h"
#include "refit.h"
#include "qnodes.h"
#include "cones.h"
#include "cullflags.h"

namespace urtd {

void free_scene(urt_context* ctx) {
  if (!ctx->scene.scene_allocs.empty()) (void)hipStreamSynchronize(touch(ctx));   // queued kernels may still read them
  ctx->scene = urt_context::Scene{};
  ctx->slab_oom_stride = 0;                                // device memory came back: the next batch may try the Result slots again
}

namespace {

// `bytes` (at least 16) of device memory that lives as long as the prepared scene
template <typename P>
int scene_alloc(urt_context* ctx, P** out, size_t bytes) {
  DeviceBuf<char>& b = ctx->scene.scene_allocs.emplace_back();
  URT_HIP(ctx, b.alloc(bytes, 16));
  *out = (P*)b.get();
  return URT_OK;
}

template <typename T>
int upload(urt_context* ctx, const std::vector<T>& v, const float4** out) {
  *out = nullptr;
  if (v.empty()) return URT_OK;
  if (int rc = scene_alloc(ctx, out, v.size() * sizeof(T))) return rc;
  // synchronous on purpose: `v` is a short-lived staging vector, and a pageable-memory hipMemcpyAsync may
  // still be reading it after this function returns
  URT_HIP(ctx, hipMemcpy(const_cast<float4*>(*out), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return URT_OK;
}

// Everything Shade (RS:388-419) derives from the material ALONE is evaluated here, once per material, with the normative
// arithmetic of include/urt_math.h in the shader's own operation order (the same functions the oracle evaluates per hit, so the
// bits are the same): the clamped albedo, the two normalised roulette chances and their sum, the Phong exponent
// alpha = pow(1000, smoothness^2), 1/(alpha+1), (alpha+2)/(alpha+1) and the two energy factors (1/chance) * colour.
// Per hit the kernel then loads 64 bytes and skips two dot products, a pow and six IEEE divisions.
//   [0] (1/diffChance) * albedo', specChance      [1] (1/specChance) * specular, specChance + diffChance
//   [2] emission, diffChance                       [3] alpha, 1/(alpha+1), (alpha+2)/(alpha+1), 0
constexpr int kMatFloats = 16;
void pack_material(const urt_RayTraceParams& m, float* dst) {
  using namespace urt;
  v3 albedo = mk3(m.color_albedo[0], m.color_albedo[1], m.color_albedo[2]);
  v3 spec = mk3(m.color_specular[0], m.color_specular[1], m.color_specular[2]);
  albedo = vmin3(mk3(1.0f, 1.0f, 1.0f) - spec, albedo);                          // RS:390
  const float third = 1.0f / 3.0f;
  float specChance = dot(spec, mk3(third, third, third));                        // RS:391-392
  float diffChance = dot(albedo, mk3(third, third, third));
  float sum = specChance + diffChance;                                           // RS:393-395
  specChance /= sum;
  diffChance /= sum;
  float alpha = f_pow(1000.0f, m.smoothness * m.smoothness);                     // RS:401
  v3 ks = (1.0f / specChance) * spec;                                            // RS:405
  v3 kd = (1.0f / diffChance) * albedo;                                          // RS:411
  dst[0] = kd.x; dst[1] = kd.y; dst[2] = kd.z; dst[3] = specChance;
  dst[4] = ks.x; dst[5] = ks.y; dst[6] = ks.z; dst[7] = specChance + diffChance;
  dst[8] = m.emission[0]; dst[9] = m.emission[1]; dst[10] = m.emission[2]; dst[11] = diffChance;
  dst[12] = alpha; dst[13] = 1.0f / (alpha + 1.0f); dst[14] = (alpha + 2) / (alpha + 1); dst[15] = 0.0f;   // RS:104, 404
}

// The albedo feature buffer's entry of a material (urt_render_aov): the clamped albedo Shade uses (RS:390), as pack_material computes it,
// and the smoothness.
constexpr int kAlbedoFloats = 4;
void pack_albedo(const urt_RayTraceParams& m, float* dst) {
  using namespace urt;
  v3 albedo = mk3(m.color_albedo[0], m.color_albedo[1], m.color_albedo[2]);
  v3 spec = mk3(m.color_specular[0], m.color_specular[1], m.color_specular[2]);
  albedo = vmin3(mk3(1.0f, 1.0f, 1.0f) - spec, albedo);                          // RS:390
  dst[0] = albedo.x; dst[1] = albedo.y; dst[2] = albedo.z; dst[3] = m.smoothness;
}

// "Masked" object-level walk (front_device.h front_masked): for a mesh heap of <= 31 nodes the walk RS:294-326 is evaluated without
// a stack.  Which nodes a ray pops depends only on the slab tests of their ancestors, and the pop order (children pushed 2i+1
// then 2i+2, so the right child is popped first) is a static pre-order of the heap.  The heap is therefore re-indexed in that
// order ("position"): the right child of the node at position p sits at p + 1, the left child at p + 2^(h-1), h = levels below and
// including p.  One bit per position: H = slab test passed, P = popped (root; children of a popped, hit, interior node — a shift
// per level), objects to test = popped leaves from the first popped-and-hit leaf on (`tests` is never reset, A.5), in position
// order = pop order.  The table appended to the device copy of the heap (float4 units; layout shared with front_device.h front_masked):
//   [0]  n_eval, levels, interior mask, exist mask          [1] leaf_any mask, leaf_valid mask, 0, 0
//   [2]  depth masks d = 0..3                                [3] left-child shifts d = 0..3
//   [4 .. 20)  per position p = 0..31: int2 {triangle-BVH root of the MeshObject, first triangle in the LDS copy of the single-leaf
//              MeshObjects or -1}
//   [20 .. 20 + 2 * n_eval)  the nodes whose slab test can matter (inside the buffer, non-empty bounds, every ancestor an interior
//              non-empty node), in position order: vmin.xyz, position bit of the parent (0 = root) | vmax.xyz, position bit
constexpr int kWalkHeaderF4 = 20;
}  // namespace
bool build_walk_table(const Buffer* heap, int n_meshes, const std::vector<int32_t>& mesh_root, const std::vector<int32_t>& small_first,
                      std::vector<float>& out) {
  out.clear();
  if (!heap || heap->count < 1 || heap->count > 31) return false;
  const int n = heap->count, D = heap_levels(n);            // complete tree of D levels holds the array
  const int N = (1 << D) - 1;
  std::vector<int> pos((size_t)N, -1), depth((size_t)N, 0);
  {   // right-first pre-order positions of the complete tree's slots
    std::vector<int> stack{0};
    int next = 0;
    while (!stack.empty()) {
      int i = stack.back(); stack.pop_back();
      pos[(size_t)i] = next++;
      if (2 * i + 2 < N) { depth[(size_t)(2 * i + 1)] = depth[(size_t)(2 * i + 2)] = depth[(size_t)i] + 1; stack.push_back(2 * i + 1); stack.push_back(2 * i + 2); }
    }
  }
  auto node = [&](int i) { urt_BVHNode nd; std::memcpy(&nd, heap->host.data() + (size_t)i * URT_STRIDE_BVHNODE, sizeof nd); return nd; };
  uint32_t imask = 0, exist = 0, leaf_any = 0, leaf_valid = 0, dm[4] = {0, 0, 0, 0};
  int32_t ls[4] = {0, 0, 0, 0};
  std::vector<int32_t> pos_tab(64, 0);
  for (int p = 0; p < 32; p++) { pos_tab[(size_t)(2 * p)] = kEmptyMeshRoot; pos_tab[(size_t)(2 * p + 1)] = -1; }   // (positions that are never tested)
  std::vector<char> live((size_t)N, 0);                      // slab test can matter
  struct Ev { int p, parent_p; urt_BVHNode nd; };
  std::vector<Ev> ev;
  for (int i = 0; i < N; i++) {
    const int p = pos[(size_t)i], d = depth[(size_t)i];
    if (d < D - 1 && d < 4) { dm[d] |= 1u << p; ls[d] = 1 << (D - d - 1); }
    if (i >= n) continue;
    urt_BVHNode nd = node(i);
    exist |= 1u << p;
    if (nd.index < 0) imask |= 1u << p; else leaf_any |= 1u << p;
    bool nonempty = !(nd.vmin[0] == nd.vmax[0] && nd.vmin[1] == nd.vmax[1] && nd.vmin[2] == nd.vmax[2]);      // RS:273
    bool parent_ok = i == 0 || (live[(size_t)((i - 1) / 2)] && node((i - 1) / 2).index < 0);
    live[(size_t)i] = nonempty && parent_ok;
    if (nd.index >= 0 && nd.index < n_meshes && mesh_root[(size_t)nd.index] != kEmptyMeshRoot) {      // a MeshObject without triangles is never tested
      leaf_valid |= 1u << p;
      pos_tab[(size_t)(2 * p)] = mesh_root[(size_t)nd.index];
      pos_tab[(size_t)(2 * p + 1)] = small_first.empty() ? -1 : small_first[(size_t)nd.index];
    }
    if (live[(size_t)i]) ev.push_back(Ev{p, i == 0 ? -1 : pos[(size_t)((i - 1) / 2)], nd});
  }
  std::sort(ev.begin(), ev.end(), [](const Ev& a, const Ev& b) { return a.p < b.p; });
  out.assign((size_t)(kWalkHeaderF4 + 2 * ev.size()) * 4, 0.0f);
  auto put = [&](size_t word, int32_t v) { std::memcpy(&out[word], &v, 4); };
  put(0, (int32_t)ev.size()); put(1, D); put(2, (int32_t)imask); put(3, (int32_t)exist);
  put(4, (int32_t)leaf_any); put(5, (int32_t)leaf_valid);
  for (int d = 0; d < 4; d++) { put(8 + (size_t)d, (int32_t)dm[d]); put(12 + (size_t)d, ls[d]); }
  for (size_t k = 0; k < 64; k++) put(16 + k, pos_tab[k]);
  for (size_t e = 0; e < ev.size(); e++) {
    float* o = out.data() + (size_t)(kWalkHeaderF4 + 2 * e) * 4;
    o[0] = ev[e].nd.vmin[0]; o[1] = ev[e].nd.vmin[1]; o[2] = ev[e].nd.vmin[2];
    int32_t pbit = ev[e].parent_p < 0 ? 0 : (int32_t)(1u << ev[e].parent_p); std::memcpy(&o[3], &pbit, 4);
    o[4] = ev[e].nd.vmax[0]; o[5] = ev[e].nd.vmax[1]; o[6] = ev[e].nd.vmax[2];
    int32_t bit = (int32_t)(1u << ev[e].p); std::memcpy(&o[7], &bit, 4);
  }
  return true;
}
namespace {

void pack_tlas(const Buffer* b, std::vector<float>& out, const std::vector<int32_t>* cull_words = nullptr) {
  out.clear();
  if (!b) return;
  out.resize((size_t)b->count * 8);
  for (int i = 0; i < b->count; i++) {
    urt_BVHNode nd;
    std::memcpy(&nd, b->host.data() + (size_t)i * URT_STRIDE_BVHNODE, sizeof nd);
    float* o = out.data() + (size_t)i * 8;
    o[0] = nd.vmin[0]; o[1] = nd.vmin[1]; o[2] = nd.vmin[2]; std::memcpy(&o[3], &nd.index, 4);
    o[4] = nd.vmax[0]; o[5] = nd.vmax[1]; o[6] = nd.vmax[2]; o[7] = 0;
    if (cull_words && (size_t)i < cull_words->size()) std::memcpy(&o[7], &(*cull_words)[(size_t)i], 4);      // (0 = never culled)
  }
}

// right-first pre-order position of every slot of the complete tree that holds an n-node heap (the pop order of RS:294-326; build_walk_table)
void heap_positions(int n, std::vector<int>& pos, std::vector<int>& depth, int* levels, int* slots) {
  const int D = heap_levels(n), N = (1 << D) - 1;
  pos.assign((size_t)N, -1); depth.assign((size_t)N, 0);
  std::vector<int> stack{0};
  int next = 0;
  while (!stack.empty()) {
    int i = stack.back(); stack.pop_back();
    pos[(size_t)i] = next++;
    if (2 * i + 2 < N) { depth[(size_t)(2 * i + 1)] = depth[(size_t)(2 * i + 2)] = depth[(size_t)i] + 1; stack.push_back(2 * i + 1); stack.push_back(2 * i + 2); }
  }
  *levels = D; *slots = N;
}

// Object-level cull (urt_math.h tlas_cull): the cull word of every heap node — non-zero for the leaves that are ELIGIBLE: a MeshObject
// with triangles that exactly one leaf of the heap names.  (A lone MeshObject gains too: a ray that leaves it behind, or meets the ground
// first, skips the round trip through the triangle-BVH phase — C3 -1.5 %, C3D -2.5 %, profiles/r04_logs/r4_ab_front_cull.log.)
// The word is the leaf's position bit of the masked walk (heaps of <= 31 nodes) or 1.
// csrc/cullflags.hip then clears the word of every leaf whose box does not contain its object's triangles.  mesh_leaf[m] = that leaf, or -1.
void cull_words(const urt_context* ctx, const Buffer* heap, int n_meshes, const std::vector<int32_t>& mesh_root, std::vector<int32_t>& words,
                std::vector<int32_t>& mesh_leaf) {
  const int n = heap ? heap->count : 0;
  words.assign((size_t)n, 0);
  mesh_leaf.assign((size_t)std::max(0, n_meshes), -1);
  if (!ctx->opt.front_cull || n_meshes < 1 || n < 1) return;
  std::vector<int> refs((size_t)n_meshes, 0);
  auto node = [&](int i) { urt_BVHNode nd; std::memcpy(&nd, heap->host.data() + (size_t)i * URT_STRIDE_BVHNODE, sizeof nd); return nd; };
  for (int i = 0; i < n; i++) { urt_BVHNode nd = node(i); if (nd.index >= 0 && nd.index < n_meshes) refs[(size_t)nd.index]++; }
  std::vector<int> pos, depth; int D = 0, N = 0;
  if (n <= 31) heap_positions(n, pos, depth, &D, &N);
  for (int i = 0; i < n; i++) {
    urt_BVHNode nd = node(i);
    if (nd.index < 0 || nd.index >= n_meshes || refs[(size_t)nd.index] != 1) continue;
    if ((size_t)nd.index >= mesh_root.size() || mesh_root[(size_t)nd.index] == kEmptyMeshRoot) continue;
    if (nd.vmin[0] == nd.vmax[0] && nd.vmin[1] == nd.vmax[1] && nd.vmin[2] == nd.vmax[2]) continue;       // RS:273: never passes the slab test, its t values are not computed
    words[(size_t)i] = n <= 31 ? (int32_t)(1u << pos[(size_t)i]) : 1;
    mesh_leaf[(size_t)nd.index] = i;
  }
}

// Upload mesh_leaf and run the verification pass over the prepared scene's triangle records (after a build and after every refit).
int verify_cull_flags(urt_context* ctx, const std::vector<int32_t>& words, const std::vector<int32_t>& mesh_leaf) {
  DevScene& S = ctx->scene.ds;
  bool any = false;
  for (int32_t w : words) any = any || w != 0;
  S.cull_any = 0;
  if (!any || S.n_mesh_tlas <= 0 || !S.mesh_tlas) return URT_OK;
  S.cull_any = 1;
  if (mesh_leaf.size() > ctx->scene.cap_mesh_leaf || !ctx->scene.d_mesh_leaf) {
    if (int rc = scene_alloc(ctx, &ctx->scene.d_mesh_leaf, mesh_leaf.size() * sizeof(int32_t))) return rc;
    ctx->scene.cap_mesh_leaf = mesh_leaf.size();
  }
  URT_HIP(ctx, hipMemcpy(ctx->scene.d_mesh_leaf, mesh_leaf.data(), mesh_leaf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  int* mask = ctx->scene.walk_f4 > 0 ? (int*)const_cast<float4*>(S.mesh_tlas + 2 * (size_t)S.n_mesh_tlas) + 6 : nullptr;      // header word [6] of the walk table behind the heap
  URT_HIP(ctx, update_cull_flags(const_cast<float4*>(S.mesh_tlas), S.n_mesh_tlas, ctx->scene.d_mesh_leaf, S.n_meshes, S.tri_verts, ctx->scene.n_scene_tris, mask, touch(ctx)));
  return URT_OK;
}

int requantize(urt_context* ctx);
// (Re)derive what the trace kernels read from the [lo, hi] nodes of the prepared scene — after a build and after every refit: the
// centre / half-extent copy (always), the normal cones in its spare dwords (option blas_cones: a moved MeshObject turns its normals) and
// the quantized copy (option qnodes).
int rederive_nodes(urt_context* ctx) {
  urt_context::Scene& C = ctx->scene;
  DevScene& S = C.ds;
  S.blas_cnodes = nullptr;
  C.cones_in_use = false;
  ctx->nodes_epoch++;                       // what was derived from the old node contents (the tile entry table) is stale
  if (C.cbuf && C.n_blas_nodes > 0) {
    URT_HIP(ctx, center_nodes(S.blas_nodes, C.n_blas_nodes, C.cbuf, touch(ctx)));
    S.blas_cnodes = C.cbuf;
    if (C.cone_rng[0] && C.cone_rng[1] && C.n_scene_tris > 0) {
      if (!C.cone_ranges)         // the topology's: found once per prepared scene
        URT_HIP(ctx, cone_ranges(S.blas_nodes, C.n_blas_nodes, std::max(1, C.scene_max_depth), C.cone_rng[0], C.cone_rng[1], &C.cone_ranges, touch(ctx)));
      URT_HIP(ctx, cone_words(C.cone_ranges, C.n_blas_nodes, S.tri_verts, C.n_scene_tris, C.cbuf, touch(ctx)));
      C.cones_in_use = true;
    }
  }
  return requantize(ctx);
}
// (Re)derive the quantized nodes from the float nodes of the prepared scene and decide whether the traversal loop uses them.
int requantize(urt_context* ctx) {
  DevScene& S = ctx->scene.ds;
  S.blas_qnodes = nullptr;
  if (ctx->opt.qnodes == 0 || !ctx->scene.qbuf || ctx->scene.n_blas_nodes <= 0) return URT_OK;
  URT_HIP(ctx, quantize_nodes(S.blas_nodes, ctx->scene.n_blas_nodes, S.mesh_root, S.n_meshes, ctx->scene.qbuf, touch(ctx)));
  float4 f[2];
  URT_HIP(ctx, hipMemcpyAsync(f, ctx->scene.qbuf, sizeof f, hipMemcpyDeviceToHost, touch(ctx)));
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
  ctx->scene.qnode_quality = f[0].w;
  // the traversal's planes are fma(2^23 + q, S, B) with S = cell / d and |1 / d| <= 1e18 (blas_rcp): 2^24 S must stay finite, so a
  // forest whose grid cell exceeds 2^43 (an extent of ~5.8e17) cannot use them, whatever the option says (tests/test_qnodes_ref.py)
  const bool fits = std::max(std::max(f[1].x, f[1].y), f[1].z) <= 8796093022208.0f;
  // one grid for the whole forest: a MeshObject that spans only a few hundred cells would have boxes of a few cells — every ray through
  // it would walk most of its tree.  Such scenes keep the float nodes (auto); "qnodes" = 1 insists.
  if (fits && (ctx->opt.qnodes == 1 || f[0].w >= 1024.0f)) S.blas_qnodes = ctx->scene.qbuf;
  return URT_OK;
}

// Update a small device array of the prepared scene: in place while it fits its allocation, else a new allocation (the old one
// stays in scene_allocs until the next full preparation).  The stream has been waited for.
int update_array(urt_context* ctx, const std::vector<float>& v, const float4** dev, size_t* cap_f4) {
  size_t need = (v.size() + 3) / 4;
  if (need == 0) { *dev = nullptr; return URT_OK; }
  if (*dev && need <= *cap_f4) {
    URT_HIP(ctx, hipMemcpy(const_cast<float4*>(*dev), v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return URT_OK;
  }
  int rc = upload(ctx, v, dev);
  if (rc == URT_OK) *cap_f4 = need;
  return rc;
}


urt_MeshObject mesh_object(const std::vector<uint8_t>& records, int i) {
  urt_MeshObject m;
  std::memcpy(&m, records.data() + (size_t)i * URT_STRIDE_MESHOBJECT, sizeof m);
  return m;
}

// The small tables of a scene, packed from the bound buffers and the roots of the triangle BVHs.  Both preparation paths pack them
// here and store them through store_scene_tables; they differ in what happens to the triangle BVHs.
struct SceneTables {
  std::vector<float> mats, albedo;              // spheres first, then mesh objects, then the ground plane (pack_material, pack_albedo)
  std::vector<float> sphere_pr;                 // position, radius
  std::vector<float> mesh_tlas, sphere_tlas;    // object-level heaps (pack_tlas); a small mesh heap's masked-walk table rides behind it (front_device.h front_masked)
  std::vector<int32_t> cull, mesh_leaf;         // cull_words
  int walk_f4 = 0, n_mesh_tlas = 0, n_sphere_tlas = 0, tlas_stack = 2;
};

int pack_scene_tables(urt_context* ctx, const Buffer* bm, const Buffer* bs, const Buffer* bmt, const Buffer* bst,
                      const std::vector<int32_t>& mesh_root, const std::vector<int32_t>& small_first, SceneTables& T) {
  const int n_meshes = bm ? bm->count : 0, n_spheres = bs ? bs->count : 0;
  T.mats.resize((size_t)(n_meshes + n_spheres + 1) * kMatFloats);
  T.albedo.resize((size_t)(n_meshes + n_spheres + 1) * kAlbedoFloats);
  auto material = [&](int slot, const urt_RayTraceParams& m) {
    pack_material(m, T.mats.data() + (size_t)slot * kMatFloats);
    pack_albedo(m, T.albedo.data() + (size_t)slot * kAlbedoFloats);
  };
  urt_RayTraceParams ground{};                                                   // RS:164-170: hard-coded material of the y = 0 plane
  ground.color_albedo[0] = 0.5f; ground.color_albedo[1] = 0.3f; ground.color_albedo[2] = 0.15f; ground.smoothness = 0.3f;
  material(n_meshes + n_spheres, ground);
  for (int m = 0; m < n_meshes; m++) material(n_spheres + m, mesh_object(bm->host, m).lighting);
  T.sphere_pr.resize((size_t)n_spheres * 4);
  for (int i = 0; i < n_spheres; i++) {
    urt_Sphere sp;
    std::memcpy(&sp, bs->host.data() + (size_t)i * URT_STRIDE_SPHERE, sizeof sp);
    float* pr = T.sphere_pr.data() + 4 * (size_t)i;
    pr[0] = sp.position[0]; pr[1] = sp.position[1]; pr[2] = sp.position[2]; pr[3] = sp.radius;
    material(i, sp.lighting);
  }
  cull_words(ctx, bmt, n_meshes, mesh_root, T.cull, T.mesh_leaf);
  pack_tlas(bmt, T.mesh_tlas, &T.cull);
  std::vector<float> walk;
  T.walk_f4 = 0;
  if (n_meshes > 0 && build_walk_table(bmt, n_meshes, mesh_root, small_first, walk)) {
    T.walk_f4 = (int)(walk.size() / 4);
    T.mesh_tlas.insert(T.mesh_tlas.end(), walk.begin(), walk.end());
  }
  pack_tlas(bst, T.sphere_tlas);
  T.n_mesh_tlas = bmt ? bmt->count : 0; T.n_sphere_tlas = bst ? bst->count : 0;
  const int lv = std::max(heap_levels(T.n_mesh_tlas), heap_levels(T.n_sphere_tlas));      // traversal stack budget (per lane, LDS)
  if (lv + 1 > 32)
    return fail(ctx, URT_ERR_SCENE, "object-level BVH deeper than the reference's 32-entry traversal stack (RS:73-74)");
  T.tlas_stack = std::max(2, lv + 1);
  return URT_OK;
}

// Every array is a whole number of float4s (16 and 4 floats per material, 4 per sphere, 8 per heap node, 4 per walk-table entry), so the
// capacity update_array records for a fresh allocation is the array's size.  The stream has been waited for.
int store_scene_tables(urt_context* ctx, const SceneTables& T) {
  urt_context::Scene& C = ctx->scene;
  DevScene& S = C.ds;
  int rc;
  if ((rc = update_array(ctx, T.mats, &S.materials, &C.cap_materials))) return rc;
  if ((rc = update_array(ctx, T.albedo, &C.aov_albedo, &C.cap_aov_albedo))) return rc;
  if ((rc = update_array(ctx, T.sphere_pr, &S.sphere_pr, &C.cap_sphere_pr))) return rc;
  C.walk_f4 = T.walk_f4;
  if ((rc = update_array(ctx, T.mesh_tlas, &S.mesh_tlas, &C.cap_mesh_tlas))) return rc;
  S.n_mesh_tlas = T.n_mesh_tlas;
  if ((rc = update_array(ctx, T.sphere_tlas, &S.sphere_tlas, &C.cap_sphere_tlas))) return rc;
  S.n_sphere_tlas = T.n_sphere_tlas;
  C.tlas_stack = T.tlas_stack;
  return URT_OK;
}

// Every preparation ends the dirty element ranges of the bound buffers: they are relative to the scene that now exists.
void clear_dirty_ranges(urt_context* ctx) {
  for (int s = 0; s < B_COUNT; s++) {
    auto it = ctx->buffers.find(ctx->bound[s]);
    if (it != ctx->buffers.end()) { it->second.dirty_first = 0; it->second.dirty_last = -1; }
  }
}

// Tree cost of every MeshObject from the (sum, root area) pairs of csrc/refit.hip tree_cost: 0 without nodes or with a root box of zero or
// non-finite area.
void costs_from_pairs(const std::vector<double>& pairs, std::vector<float>& out) {
  out.assign(pairs.size() / 2, 0.0f);
  for (size_t m = 0; m < out.size(); m++) {
    const double sum = pairs[2 * m], area = pairs[2 * m + 1];
    if (area > 0.0 && std::isfinite(area) && std::isfinite(sum)) out[m] = (float)(sum / area);
  }
}

// The baseline costs (measured on the stream by the full preparation) reach the host at the first need.  Waits for the stream.
int fetch_cost_base(urt_context* ctx) {
  urt_context::Scene& C = ctx->scene;
  const size_t n = (size_t)std::max(0, C.ds.n_meshes);
  if (C.h_cost_base.size() == n) return URT_OK;
  std::vector<double> pairs(2 * n, 0.0);
  if (n > 0 && C.refit.cost_base) {
    URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
    URT_HIP(ctx, hipMemcpy(pairs.data(), C.refit.cost_base, pairs.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  costs_from_pairs(pairs, C.h_cost_base);
  return URT_OK;
}

// The costs of the trees as they are now.  Waits for the stream.
int measure_cost_now(urt_context* ctx, std::vector<float>& now) {
  urt_context::Scene& C = ctx->scene;
  const size_t n = (size_t)std::max(0, C.ds.n_meshes);
  std::vector<double> pairs(2 * n, 0.0);
  if (n > 0 && C.refit.cost_now && C.refit.ready) {
    URT_HIP(ctx, tree_cost(C.ds.blas_nodes, C.n_blas_nodes, C.refit.parent, C.refit.node_mesh, (int)n, C.refit.cost_now, touch(ctx)));
    URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));
    URT_HIP(ctx, hipMemcpy(pairs.data(), C.refit.cost_now, pairs.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  costs_from_pairs(pairs, now);
  return URT_OK;
}

// The dynamic-scene path (RM:215-230: a moved object makes the reference re-upload every buffer).  When the only contents that changed
// since the scene was prepared are those of _MeshObjects / _MeshBVH / _Spheres / _SphereBVH — same counts, same index ranges per
// MeshObject — the device scene is UPDATED: materials, object-level heaps and sphere tables are re-packed (a few KB), and every
// MeshObject whose localToWorldMatrix changed keeps its triangle BVH's topology: its triangle records and boxes are recomputed on the
// GPU (csrc/refit.hip).  Changed contents of _Vertices / _Normals — same counts, _Indices untouched — are taken the same way (option
// "refit_vertices"): only the dirty element range is copied into the device copy, a MeshObject whose vertex span meets the dirty range of
// _Vertices is DEFORMED and refitted together with the moved ones, and one whose span meets the dirty range of _Normals has its shading
// normals gathered again.  Returns 1 when the change is not of that kind, or when option "refit_rebuild_pct" finds the refitted tree of a
// deformed MeshObject too costly (the caller prepares from scratch).
int prepare_incremental(urt_context* ctx) {
  const unsigned int small = (1u << B_MESHOBJECTS) | (1u << B_MESHBVH) | (1u << B_SPHERES) | (1u << B_SPHEREBVH);
  const unsigned int geometry = (1u << B_VERTICES) | (1u << B_NORMALS);
  urt_context::Scene& C = ctx->scene;
  if (!ctx->opt.refit || ctx->dirty_full || C.scene_allocs.empty()) return 1;
  if (ctx->dirty_slots & ~(small | (ctx->opt.refit_vertices ? geometry : 0u))) return 1;
  if (int rc = sync_bound_hosts(ctx, small)) return rc;     // the small tables are packed from the host copies
  DevScene& S = C.ds;
  const Buffer* bm = bound_buffer(ctx, B_MESHOBJECTS);
  const Buffer* bs = bound_buffer(ctx, B_SPHERES);
  const int n_meshes = bm ? bm->count : 0, n_spheres = bs ? bs->count : 0;
  if (n_meshes != S.n_meshes || n_spheres != S.n_spheres) return 1;
  if ((size_t)n_meshes * URT_STRIDE_MESHOBJECT != C.prev_mesh_objects.size()) return 1;
  // changed vertices / normals: the buffers must be the ones (by size) the scene was prepared from
  const Buffer* bv = (ctx->dirty_slots & (1u << B_VERTICES)) ? bound_buffer(ctx, B_VERTICES) : nullptr;
  const Buffer* bn = (ctx->dirty_slots & (1u << B_NORMALS)) ? bound_buffer(ctx, B_NORMALS) : nullptr;
  if (ctx->dirty_slots & geometry) {
    const Buffer* v = bound_buffer(ctx, B_VERTICES); const Buffer* n = bound_buffer(ctx, B_NORMALS);
    if ((v ? v->count : 0) != C.n_vertices || (n ? n->count : 0) != C.n_normals) return 1;
    if (!C.refit.ready || C.n_scene_tris <= 0 || C.h_vert_lo.size() != (size_t)n_meshes) return 1;
    if (bv && (!C.refit.vertices || bv->dirty_last < bv->dirty_first)) return 1;
    if (bn && (!C.refit.normals || !C.refit.renormed || bn->dirty_last < bn->dirty_first)) return 1;
  }
  auto t_begin = std::chrono::steady_clock::now();
  std::vector<int32_t> moved((size_t)n_meshes, 0), renormed((size_t)n_meshes, 0);
  std::vector<char> deformed((size_t)n_meshes, 0);
  std::vector<float> matrices((size_t)n_meshes * 16, 0.0f);
  int n_moved = 0, n_deformed = 0, n_renormed = 0;
  for (int m = 0; m < n_meshes; m++) {
    const urt_MeshObject a = mesh_object(C.prev_mesh_objects, m), b = mesh_object(bm->host, m);
    if (a.indices_offset != b.indices_offset || a.indices_count != b.indices_count) return 1;
    std::memcpy(&matrices[(size_t)m * 16], b.localToWorldMatrix, 64);
    if (b.indices_count < 3) continue;
    bool refit = std::memcmp(a.localToWorldMatrix, b.localToWorldMatrix, 64) != 0;
    if (bv || bn) {
      const int lo = C.h_vert_lo[(size_t)m], hi = C.h_vert_hi[(size_t)m];      // (conservative: a vertex inside the span that no index names counts)
      if (bv && lo <= bv->dirty_last && hi >= bv->dirty_first) { deformed[(size_t)m] = 1; n_deformed++; refit = true; }
      if (bn && lo <= bn->dirty_last && hi >= bn->dirty_first) { renormed[(size_t)m] = 1; n_renormed++; }
    }
    if (refit) { moved[(size_t)m] = 1; n_moved++; }
  }
  if (n_moved > 0 && (!C.refit.ready || C.n_scene_tris <= 0)) return 1;
  URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));           // frames in flight read the arrays that are about to change
  int rc;
  SceneTables T;
  if ((rc = pack_scene_tables(ctx, bm, bs, bound_buffer(ctx, B_MESHBVH), bound_buffer(ctx, B_SPHEREBVH), C.h_mesh_root, C.h_small_first, T))) return rc;
  if ((rc = store_scene_tables(ctx, T))) return rc;
  // the dirty element ranges go into the device copies, on the stream, behind the wait above and ahead of the kernels that read them.
  // From a buffer with a device mirror (current by construction): device to device, and the host is not involved.  Else from the buffer's
  // own host copy; the stream is waited for below, before a later SetData can change it.
  uint64_t copied = 0, from_host = 0;
  auto copy_dirty = [&](const Buffer* b, const float* scene_copy) -> hipError_t {
    const size_t at = (size_t)b->dirty_first * 12, bytes = (size_t)(b->dirty_last - b->dirty_first + 1) * 12;
    copied += bytes;
    if (b->mirror) return hipMemcpyAsync((char*)const_cast<float*>(scene_copy) + at, b->mirror.get() + at, bytes, hipMemcpyDeviceToDevice, touch(ctx));
    from_host += bytes;
    return hipMemcpyAsync((char*)const_cast<float*>(scene_copy) + at, b->host.data() + at, bytes, hipMemcpyHostToDevice, touch(ctx));
  };
  if (bv) URT_HIP(ctx, copy_dirty(bv, C.refit.vertices));
  if (bn) URT_HIP(ctx, copy_dirty(bn, C.refit.normals));
  if (n_moved > 0) {
    URT_HIP(ctx, hipMemcpy(C.refit.matrices, matrices.data(), matrices.size() * sizeof(float), hipMemcpyHostToDevice));
    URT_HIP(ctx, hipMemcpy(C.refit.moved, moved.data(), moved.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    URT_HIP(ctx, refit_moved(const_cast<float4*>(S.blas_nodes), C.n_blas_nodes, const_cast<float4*>(S.tri_verts), C.n_scene_tris,
                             C.refit.vertices, C.refit.indices, C.refit.depth, std::max(0, C.scene_max_depth - 1), C.refit.node_mesh,
                             C.refit.matrices, C.refit.moved, C.refit.ext, n_meshes, C.refit.cbox, touch(ctx)));
  }
  if (n_renormed > 0 && S.tri_norms) {
    URT_HIP(ctx, hipMemcpy(C.refit.renormed, renormed.data(), renormed.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    URT_HIP(ctx, refit_norms(const_cast<float4*>(S.tri_norms), S.tri_verts, C.n_scene_tris, C.refit.normals, C.refit.indices, C.refit.renormed, touch(ctx)));
  }
  if (n_moved > 0 && (rc = rederive_nodes(ctx))) return rc;
  if ((rc = verify_cull_flags(ctx, T.cull, T.mesh_leaf))) return rc;       // against the (refitted) triangle records
  if (from_host > 0) URT_HIP(ctx, hipStreamSynchronize(touch(ctx)));         // the copies have left the buffers' host memory
  if (n_deformed > 0) {
    // a refit keeps the topology, and a large deformation can make it a bad one: the cost of each deformed MeshObject's refitted tree
    // against what it was when the tree was built
    std::vector<float> now;
    if ((rc = fetch_cost_base(ctx))) return rc;
    if ((rc = measure_cost_now(ctx, now))) return rc;
    float worst = 0.0f;
    for (int m = 0; m < n_meshes; m++)
      if (deformed[(size_t)m] && C.h_cost_base[(size_t)m] > 0.0f) worst = std::max(worst, now[(size_t)m] / C.h_cost_base[(size_t)m]);
    ctx->last_cost_ratio = worst;
    if (ctx->opt.refit_rebuild_pct > 0 && worst * 100.0f > (float)ctx->opt.refit_rebuild_pct) {
      ctx->forced_rebuilds++;
      return 1;                                               // the full preparation reads the buffers, not what was refitted here
    }
  }
  ctx->refitted_meshes += (uint64_t)n_moved;
  ctx->deformed_meshes += (uint64_t)n_deformed; ctx->renormed_meshes += (uint64_t)n_renormed; ctx->deform_bytes += copied;
  if (bm) C.prev_mesh_objects.assign(bm->host.begin(), bm->host.begin() + (ptrdiff_t)((size_t)n_meshes * URT_STRIDE_MESHOBJECT));
  clear_dirty_ranges(ctx);
  ctx->scene_dirty = false; ctx->dirty_slots = 0; ctx->dirty_full = false;
  ctx->scene_epoch++;
  ctx->incremental_preps++;
  ctx->last_prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return URT_OK;
}

}  // namespace

// Derive the device scene from the bound ComputeBuffers (runs at the first dispatch after a change;
// the reference pays the equivalent in RebuildTrees -> SetData, RM:725-746).
int prepare_scene(urt_context* ctx) {
  {
    int rc = prepare_incremental(ctx);
    if (rc != 1) return rc;                                 // updated in place (or failed)
  }
  // Everything below reads the host copies, so device-written data come down first — except, with option "prepare_device", the three
  // geometry buffers: the GPU builder takes them from their mirrors, their host copies are not read and their stale ranges stay as they are.
  const bool from_device = ctx->opt.prepare_device != 0;
  const unsigned int geometry_slots = (1u << B_VERTICES) | (1u << B_INDICES) | (1u << B_NORMALS);
  if (int rc = sync_bound_hosts(ctx, ((1u << B_COUNT) - 1u) & ~(from_device ? geometry_slots : 0u))) return rc;
  free_scene(ctx);
  urt_context::Scene& C = ctx->scene;
  DevScene& S = C.ds;
  const Buffer* bm = bound_buffer(ctx, B_MESHOBJECTS);
  const Buffer* bv = bound_buffer(ctx, B_VERTICES);
  const Buffer* bi = bound_buffer(ctx, B_INDICES);
  const Buffer* bn = bound_buffer(ctx, B_NORMALS);
  const Buffer* bs = bound_buffer(ctx, B_SPHERES);

  int rc;
  const int n_meshes = bm ? bm->count : 0, n_spheres = bs ? bs->count : 0;
  // meshes: the triangle BVH ("BLAS") of every MeshObject, by the host SAH builder or by the GPU LBVH builder
  auto t_begin = std::chrono::steady_clock::now();
  std::vector<int32_t> mesh_root_host, small_first;
  std::vector<int32_t> span_lo_hi;                           // option "prepare_device": (lo, hi) per MeshObject from csrc/index_span.hip
  int blas_max_depth = 0;
  size_t n_blas_nodes = 0, n_tris = 0;
  if (n_meshes > 0) {
    std::vector<int32_t> offs((size_t)n_meshes), cnts((size_t)n_meshes);
    long tris = 0;
    for (int m = 0; m < n_meshes; m++) {
      const urt_MeshObject mo = mesh_object(bm->host, m);
      offs[(size_t)m] = mo.indices_offset; cnts[(size_t)m] = mo.indices_count; tris += std::max(0, mo.indices_count) / 3;
    }
    const float4* p;
    // auto: the host builder up to kGpuBuildTriangles triangles (C3's 69,600: 12 ms on the host, 6 on the GPU — and small scenes are what the
    // per-MeshObject host cache is good at), the GPU's binned SAH beyond (C4 300 k: 32 -> 10 ms, C5 983 k: 80 -> 15 ms; same trees, same frames)
    constexpr long kGpuBuildTriangles = 200000;
    int builder = ctx->opt.blas_builder;
    if (builder < 0) builder = tris >= kGpuBuildTriangles ? 3 : 0;
    if (from_device && builder < 1) builder = 3;             // the host builder is host-fed; pixels do not depend on the tree
    ctx->last_builder = builder;
    if (builder >= 1) {
      // device copies of the buffers exactly as SetData delivered them; the whole build runs on the GPU (csrc/lbvh.hip)
      DeviceBuf<char> raw;
      size_t b_mo = ((size_t)n_meshes * URT_STRIDE_MESHOBJECT + 255) & ~(size_t)255;
      size_t b_v = bv ? (((size_t)bv->count * 12 + 255) & ~(size_t)255) : 0, b_i = bi ? (((size_t)bi->count * 4 + 255) & ~(size_t)255) : 0;
      size_t b_n = bn ? (((size_t)bn->count * 12 + 255) & ~(size_t)255) : 0;
      URT_HIP(ctx, raw.alloc(b_mo + b_v + b_i + b_n + 256));
      char* rb = raw.get();
      // A geometry buffer reaches the scene's own copy from its host copy — or, with option "prepare_device", from its mirror: device to
      // device on the stream, ahead of the build; the mirror is current by construction, the host copy may be stale and is not read.  (A buffer
      // without a mirror has never been written on the device: its host copy is current.)  The scene never aliases a mirror: frames in
      // flight and the refit read these copies.
      auto feed = [&](const Buffer* b, char* dst, size_t bytes) -> hipError_t {
        if (from_device && b->mirror) return hipMemcpyAsync(dst, b->mirror.get(), bytes, hipMemcpyDeviceToDevice, touch(ctx));
        return hipMemcpy(dst, b->host.data(), bytes, hipMemcpyHostToDevice);
      };
      hipError_t e = hipMemcpy(rb, bm->host.data(), (size_t)n_meshes * URT_STRIDE_MESHOBJECT, hipMemcpyHostToDevice);
      if (e == hipSuccess && bv) e = feed(bv, rb + b_mo, (size_t)bv->count * 12);
      if (e == hipSuccess && bi) e = feed(bi, rb + b_mo + b_v, (size_t)bi->count * 4);
      if (e == hipSuccess && bn) e = feed(bn, rb + b_mo + b_v + b_i, (size_t)bn->count * 12);
      if (e != hipSuccess) return fail(ctx, URT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
      // The vertex spans of a device-fed preparation (kept below for prepare_incremental) come from the scene's copy of _Indices
      // (csrc/index_span.hip): queued here, ahead of the build, and read back after the wait the build ends with.  Ranges outside _Indices
      // queue nothing: the build refuses them.
      DeviceBuf<char> span_mem;
      std::vector<SpanItem> span_tab;
      Event span_t0, span_t1;
      size_t b_tab = 0;
      bool spans_queued = false;
      if (from_device && ctx->opt.refit && tris > 0 && bv && bi && span_items(offs.data(), cnts.data(), n_meshes, bi->count, span_tab)) {
        b_tab = (span_tab.size() * sizeof(SpanItem) + 255) & ~(size_t)255;
        URT_HIP(ctx, span_mem.alloc(b_tab + (size_t)n_meshes * 8));
        URT_HIP(ctx, hipMemcpy(span_mem.get(), span_tab.data(), span_tab.size() * sizeof(SpanItem), hipMemcpyHostToDevice));
        if (ctx->opt.time_dispatch) {
          URT_HIP(ctx, span_t0.create(hipEventDefault)); URT_HIP(ctx, span_t1.create(hipEventDefault));
          URT_HIP(ctx, hipEventRecord(span_t0.get(), touch(ctx)));
        }
        URT_HIP(ctx, index_spans((const int32_t*)(rb + b_mo + b_v), (const SpanItem*)span_mem.get(), (int)span_tab.size(),
                                 (int32_t*)(span_mem.get() + b_tab), n_meshes, touch(ctx)));
        if (span_t1) URT_HIP(ctx, hipEventRecord(span_t1.get(), touch(ctx)));
        spans_queued = true;
      }
      LbvhInput in;
      in.mesh_objects = (const uint8_t*)rb; in.n_meshes = n_meshes;
      in.vertices = bv ? (const float*)(rb + b_mo) : nullptr; in.n_vertices = bv ? bv->count : 0;
      in.indices = bi ? (const int32_t*)(rb + b_mo + b_v) : nullptr; in.n_indices = bi ? bi->count : 0;
      in.normals = bn ? (const float*)(rb + b_mo + b_v + b_i) : nullptr; in.n_normals = bn ? bn->count : 0;
      in.h_offsets = offs.data(); in.h_counts = cnts.data(); in.leaf_max = get_blas_leaf_max(); in.depth_budget = builder == 2; in.depth_slack = ctx->opt.lbvh_slack; in.sah = builder == 3;
      LbvhOutput o;
      std::string err;
      rc = lbvh_build(in, touch(ctx), o, err);
      if (rc) return fail(ctx, rc, err);
      if (spans_queued) {                                                  // (the build has waited for the stream)
        span_lo_hi.resize((size_t)n_meshes * 2);
        URT_HIP(ctx, hipMemcpy(span_lo_hi.data(), span_mem.get() + b_tab, span_lo_hi.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        ctx->last_span_ms = 0;
        if (span_t1) URT_HIP(ctx, hipEventElapsedTime(&ctx->last_span_ms, span_t0.get(), span_t1.get()));
      }
      ctx->scene.scene_allocs.push_back(std::move(raw));                // _Vertices / _Indices stay resident: a moved MeshObject is refitted from them
      ctx->scene.refit.vertices = in.vertices; ctx->scene.refit.indices = in.indices; ctx->scene.refit.normals = in.normals;
      for (DeviceBuf<char>& a : o.allocs) ctx->scene.scene_allocs.push_back(std::move(a));
      S.mesh_root = o.mesh_root; S.blas_nodes = o.nodes; S.tri_verts = o.tri_verts; S.tri_norms = o.tri_norms;
      mesh_root_host = o.h_mesh_root; blas_max_depth = o.max_depth; n_blas_nodes = (size_t)o.n_nodes; n_tris = (size_t)o.n_tris;
    } else {
      BlasResult blas;
      std::string err;
      if (!build_blas(bm->host.data(), n_meshes, bv ? (const float*)bv->host.data() : nullptr, bv ? bv->count : 0,
                      bi ? (const int32_t*)bi->host.data() : nullptr, bi ? bi->count : 0,
                      bn ? (const float*)bn->host.data() : nullptr, bn ? bn->count : 0, blas, err, &ctx->blas_cache))
        return fail(ctx, URT_ERR_SCENE, err);
      if ((rc = upload(ctx, blas.mesh_root, &p))) return rc; S.mesh_root = (const int32_t*)p;
      if ((rc = upload(ctx, blas.nodes, &p))) return rc; S.blas_nodes = p;
      if ((rc = upload(ctx, blas.tri_verts, &p))) return rc; S.tri_verts = p;
      if ((rc = upload(ctx, blas.tri_norms, &p))) return rc; S.tri_norms = p;
      mesh_root_host = blas.mesh_root; blas_max_depth = blas.max_depth; n_blas_nodes = blas.nodes.size() / kBlasNodeFloats; n_tris = blas.tri_slot.size();
    }
    {   // single-leaf MeshObjects: where their triangles sit in the LDS copy (kernels.hip k_sched prologue)
      small_first.assign((size_t)n_meshes, -1);
      int n_small = 0;
      for (int m = 0; m < n_meshes; m++) {
        int32_t r = mesh_root_host[(size_t)m];
        if (r < 0 && r != (int32_t)0x80000000) { small_first[(size_t)m] = n_small; n_small += (int)((~(uint32_t)r) & 7u) + 1; }
      }
      if (n_small > 0 && n_small <= 64) {
        if ((rc = upload(ctx, small_first, &p))) return rc;
        S.mesh_small_first = (const int32_t*)p; S.n_small = n_small;
      } else small_first.assign((size_t)n_meshes, -1);
    }
  }
  S.n_meshes = n_meshes; S.n_spheres = n_spheres;
  // materials, spheres, object-level BVHs and the object-level traversal stack budget
  SceneTables T;
  if ((rc = pack_scene_tables(ctx, bm, bs, bound_buffer(ctx, B_MESHBVH), bound_buffer(ctx, B_SPHEREBVH), mesh_root_host, small_first, T))) return rc;
  if ((rc = store_scene_tables(ctx, T))) return rc;
  // triangle-BVH traversal stack budget (per lane, LDS)
  if (n_blas_nodes >= (1u << 26)) return fail(ctx, URT_ERR_SCENE, "triangle BVH larger than 2^26 nodes (4 GiB)");   // kernels address nodes by 32-bit byte offsets
  if ((uint64_t)n_tris * 48ull >= (1ull << 32)) return fail(ctx, URT_ERR_SCENE, "more than 2^32 / 48 triangles (4 GiB of triangle records)");   // 32-bit byte offsets as well
  C.blas_stack = std::max(2, blas_max_depth + 1) + 1;      // + the sentinel entry below the stack (trace_device.h blas_node_eval_ptr)
  C.n_blas_nodes = (int)std::min<size_t>(0x7fffffff, n_blas_nodes);
  C.n_scene_tris = (int)n_tris; C.scene_max_depth = blas_max_depth;
  if ((rc = verify_cull_flags(ctx, T.cull, T.mesh_leaf))) return rc;
  // a ray with NaN components passes every slab test and walks the whole tree once: (nodes + leaves) trips per lane, and the
  // majority vote can make a lane wait a trip for every trip it runs; 8x that is a bound no correct traversal reaches
  ctx->scene.watchdog_steps = (unsigned int)std::min<size_t>(0x7fffffffu, 8 * (n_blas_nodes + n_tris) + 4096);
  if ((size_t)(ctx->scene.tlas_stack + ctx->scene.blas_stack) * 64 * 4 * sizeof(int) > 150 * 1024)   // 4-wave workgroup; a CU has 160 KiB
    return fail(ctx, URT_ERR_SCENE, "traversal stacks exceed the LDS of a compute unit");
  if (n_blas_nodes > 0) {                                     // the copy of the nodes the trace kernels traverse: child boxes as (centre, half extent)
    if ((rc = scene_alloc(ctx, &ctx->scene.cbuf, 4 * n_blas_nodes * sizeof(float4)))) return rc;
  }
  if (ctx->opt.blas_cones != 0 && n_blas_nodes > 0 && n_tris > 0) {      // normal cones (csrc/cones.hip): the children's triangle ranges, 2 x 16 B per node
    if ((rc = scene_alloc(ctx, &ctx->scene.cone_rng[0], n_blas_nodes * sizeof(int4)))) return rc;
    if ((rc = scene_alloc(ctx, &ctx->scene.cone_rng[1], n_blas_nodes * sizeof(int4)))) return rc;
  }
  if (ctx->opt.qnodes != 0 && n_blas_nodes > 0) {             // 32-byte quantized nodes for the traversal loop (csrc/qnodes.hip)
    if ((rc = scene_alloc(ctx, &ctx->scene.qbuf, (2 + 2 * n_blas_nodes) * sizeof(float4)))) return rc;
  }
  if ((rc = rederive_nodes(ctx))) return rc;
  // what a later in-place update needs (prepare_incremental): the records this scene was prepared from, and — when it has triangle
  // BVHs — device copies of _Vertices / _Indices plus every node's parent and MeshObject (csrc/refit.hip)
  if (bm) C.prev_mesh_objects.assign(bm->host.begin(), bm->host.begin() + (ptrdiff_t)((size_t)n_meshes * URT_STRIDE_MESHOBJECT));
  ctx->scene.h_mesh_root = mesh_root_host; ctx->scene.h_small_first = small_first;
  if (ctx->opt.refit && n_meshes > 0 && n_tris > 0 && bv && bi) {
    urt_context::Scene::RefitAux& R = ctx->scene.refit;
    if (!R.vertices) {                                        // (the GPU builder has left its copies in place)
      float* dv = nullptr; int32_t* di = nullptr;
      if ((rc = scene_alloc(ctx, &dv, (size_t)bv->count * 12))) return rc;
      if ((rc = scene_alloc(ctx, &di, (size_t)bi->count * 4))) return rc;
      URT_HIP(ctx, hipMemcpy(dv, bv->host.data(), (size_t)bv->count * 12, hipMemcpyHostToDevice));
      URT_HIP(ctx, hipMemcpy(di, bi->host.data(), (size_t)bi->count * 4, hipMemcpyHostToDevice));
      R.vertices = dv; R.indices = di;
      if (bn) {
        float* dn = nullptr;
        if ((rc = scene_alloc(ctx, &dn, (size_t)bn->count * 12))) return rc;
        URT_HIP(ctx, hipMemcpy(dn, bn->host.data(), (size_t)bn->count * 12, hipMemcpyHostToDevice));
        R.normals = dn;
      }
    }
    {   // the span of vertices every MeshObject's index range refers to: a later SetData of _Vertices / _Normals deforms the MeshObjects
        // whose span its dirty range meets (prepare_incremental).  The builders have checked the ranges and the indices.
      C.h_vert_lo.assign((size_t)n_meshes, 0); C.h_vert_hi.assign((size_t)n_meshes, -1);
      if (from_device && span_lo_hi.size() != 2 * (size_t)n_meshes)      // (the pass above was queued under this block's own condition)
        return fail(ctx, URT_ERR_SCENE, "prepare_device: the vertex spans of the MeshObjects were not computed");
      const int32_t* idx = from_device ? nullptr : (const int32_t*)bi->host.data();      // the host copy of _Indices may be stale: not read
      for (int m = 0; m < n_meshes && from_device; m++) { C.h_vert_lo[(size_t)m] = span_lo_hi[2 * (size_t)m]; C.h_vert_hi[(size_t)m] = span_lo_hi[2 * (size_t)m + 1]; }
      for (int m = 0; m < n_meshes && !from_device; m++) {
        const urt_MeshObject mo = mesh_object(bm->host, m);
        int32_t lo = INT32_MAX, hi = -1;
        for (long i = mo.indices_offset, e = (long)mo.indices_offset + (long)(mo.indices_count / 3) * 3; i < e; i++) { lo = std::min(lo, idx[i]); hi = std::max(hi, idx[i]); }
        C.h_vert_lo[(size_t)m] = lo; C.h_vert_hi[(size_t)m] = hi;
      }
    }
    size_t nn = std::max<size_t>(1, n_blas_nodes);
    if ((rc = scene_alloc(ctx, &R.parent, nn * 4))) return rc;
    if ((rc = scene_alloc(ctx, &R.node_mesh, nn * 4))) return rc;
    if ((rc = scene_alloc(ctx, &R.cbox, nn * 64))) return rc;
    if ((rc = scene_alloc(ctx, &R.depth, nn * 4))) return rc;
    if ((rc = scene_alloc(ctx, &R.ext, (size_t)n_meshes * 4))) return rc;
    if ((rc = scene_alloc(ctx, &R.matrices, (size_t)n_meshes * 64))) return rc;
    if ((rc = scene_alloc(ctx, &R.moved, (size_t)n_meshes * 4))) return rc;
    if ((rc = scene_alloc(ctx, &R.renormed, (size_t)n_meshes * 4))) return rc;
    if ((rc = scene_alloc(ctx, &R.cost_base, (size_t)n_meshes * 16))) return rc;
    if ((rc = scene_alloc(ctx, &R.cost_now, (size_t)n_meshes * 16))) return rc;
    URT_HIP(ctx, refit_prepare(S.blas_nodes, (int)n_blas_nodes, S.tri_verts, R.parent, R.node_mesh, R.depth, touch(ctx)));
    // the cost of every tree as built: the baseline a deformed MeshObject's refitted tree is held against (read back when first needed)
    URT_HIP(ctx, tree_cost(S.blas_nodes, (int)n_blas_nodes, R.parent, R.node_mesh, n_meshes, R.cost_base, touch(ctx)));
    R.ready = true;
  }
  C.n_vertices = bv ? bv->count : 0; C.n_normals = bn ? bn->count : 0;
  clear_dirty_ranges(ctx);
  ctx->scene_dirty = false; ctx->dirty_slots = 0; ctx->dirty_full = false;
  ctx->scene_epoch++;
  ctx->full_preps++; ctx->device_preps += from_device ? 1u : 0u;
  ctx->last_prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return URT_OK;
}

// urt_debug_scene_cost: per MeshObject the cost of its tree now and at the last full preparation (all 0 without "refit": nothing is kept).
int scene_cost(urt_context* ctx, std::vector<float>& now, std::vector<float>& base) {
  if (int rc = fetch_cost_base(ctx)) return rc;
  base = ctx->scene.h_cost_base;
  return measure_cost_now(ctx, now);
}

}  // namespace urtd
