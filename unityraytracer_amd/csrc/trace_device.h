// trace_device.h — the device functions of one ray's trace that the frame kernels (kernels*.hip) and the single-ray kernels outside a
// frame (query.hip, aov.hip, radiance.hip) share: the hit record, the object-level slab tests and cull, sphere / triangle / leaf
// intersection, the triangle-BVH node steps, the per-MeshObject traversal, Trace() itself (trace_ray), its per-lane LDS stacks and the
// streaming store of a result.  Internal to the library; included by .hip translation units only, after the kernels' own headers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urt_math.h"
#include "urt_device.h"

using namespace urt;
using namespace urtd;

namespace {

struct LocalCounters {
  unsigned int rays = 0, tlas_nodes = 0, blas_nodes = 0, tri_tests = 0, sphere_tests = 0;
  unsigned int hit_tri = 0, hit_sphere = 0, hit_ground = 0, hit_sky = 0, pixels = 0;
};

struct HitRec {
  float t;     // distance, +inf = miss
  int kid;     // id << 2 | kind;  kind: 0 none, 1 ground plane, 2 sphere, 3 triangle;  id: sphere index, or leaf-order triangle slot
  float u, v;  // barycentrics of a triangle hit
  __device__ __forceinline__ int kind() const { return kid & 3; }
  __device__ __forceinline__ int id() const { return (int)((unsigned)kid >> 2); }
  __device__ __forceinline__ void set(int kind, int id) { kid = (id << 2) | kind; }
};

__device__ __forceinline__ v3 xyz(float4 q) { return mk3(q.x, q.y, q.z); }
// wave64 vote straight from the lane predicate (HIP's wballot(int) first materialises the predicate as 0/1 in a VGPR and
// compares it again: two VALU instructions per vote, and the scheduler votes several times per trip)
__device__ __forceinline__ unsigned long long wballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int as_int(float f) { return __builtin_bit_cast(int, f); }
__device__ __forceinline__ float as_float(int i) { return __builtin_bit_cast(float, i); }

// ---------------------------------------------------------------------------------------------------
// object-level BVH (the reference's implicit heap) — RS:271-291 slab test, RS:294-361 traversal
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool tlas_slab(float4 a, float4 b, v3 o, v3 rcp) {
  if (a.x == b.x && a.y == b.y && a.z == b.z) return false;      // RS:273 empty node
  float t_min = -kFLOAT_MAX, t_max = kFLOAT_MAX;
  float t1 = (a.x - o.x) * rcp.x, t2 = (b.x - o.x) * rcp.x;
  t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
  t1 = (a.y - o.y) * rcp.y; t2 = (b.y - o.y) * rcp.y;
  t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
  t1 = (a.z - o.z) * rcp.z; t2 = (b.z - o.z) * rcp.z;
  t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
  return t_max >= t_min;
}

// the same, handing out the t_min / t_max it compared (0, 0 for an empty node): what the object-level cull looks at (urt_math.h tlas_cull)
__device__ __forceinline__ bool tlas_slab_t(float4 a, float4 b, v3 o, v3 rcp, float& t_min, float& t_max) {
  t_min = 0.0f; t_max = 0.0f;
  if (a.x == b.x && a.y == b.y && a.z == b.z) return false;      // RS:273 empty node
  t_min = -kFLOAT_MAX; t_max = kFLOAT_MAX;
  float t1 = (a.x - o.x) * rcp.x, t2 = (b.x - o.x) * rcp.x;
  t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
  t1 = (a.y - o.y) * rcp.y; t2 = (b.y - o.y) * rcp.y;
  t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
  t1 = (a.z - o.z) * rcp.z; t2 = (b.z - o.z) * rcp.z;
  t_min = f_max(t_min, f_min(t1, t2)); t_max = f_min(t_max, f_max(t1, t2));
  return t_max >= t_min;
}
// Object-level cull: the leaf's cull word (second float4 of the packed node, .w) is non-zero only when the library has verified that the
// leaf's box contains the object's triangles (csrc/cullflags.hip); then the object is skipped when the reference's own slab values say the
// ray passes the box, or the box lies behind the origin or beyond the ground-plane hit, by a margin (urt_math.h tlas_cull)
__device__ __forceinline__ bool leaf_culled(float4 b, float t_min, float t_max, float t_ground) {
  return as_int(b.w) != 0 && tlas_cull(t_min, t_max, t_ground);
}

// RS:175-196 without the material copy (fetched at shading time)
template <bool COUNT>
__device__ __forceinline__ void intersect_sphere(const DevScene& S, int idx, v3 o, v3 d, HitRec& best, LocalCounters& lc,
                                                 const float4* lds_pr = nullptr) {
  if (COUNT) lc.sphere_tests++;
  float4 pr;
  if (lds_pr) pr = lds_pr[idx]; else pr = S.sphere_pr[idx];
  v3 dd = o - xyz(pr);
  float p1 = -dot(d, dd);
  float p2sqr = p1 * p1 - dot(dd, dd) + pr.w * pr.w;
  if (p2sqr < 0) return;
  float p2 = f_sqrt(p2sqr);
  float t = p1 - p2 > 0 ? p1 - p2 : p1 + p2;
  if (t > 0 && t < best.t) { best.t = t; best.set(2, idx); }
}

// The triangles of one BVH leaf: Moller-Trumbore with back-face culling, RS:199-234 (edge1/edge2 pre-subtracted on
// upload), and the closer-hit rule RS:251 extended by "equal t inside one IntersectMeshObject call goes to the lower
// index slot" (A.4) — `best_i` is the index slot of a hit made in THIS call, or -1.
template <bool COUNT>
__device__ __forceinline__ void test_triangle(float4 r0, float4 r1, float4 r2, int slot_in_leaf_order, v3 o, v3 d, HitRec& best, int& best_i,
                                              LocalCounters& lc) {
  if (COUNT) lc.tri_tests++;
  v3 edge1 = xyz(r1), edge2 = xyz(r2);
  v3 pvec = cross(d, edge2);
  float det = dot(edge1, pvec);
  if (det < kEPSILON) return;
  float inv_det = 1.0f / det;
  v3 tvec = o - xyz(r0);
  float u = dot(tvec, pvec) * inv_det;
  if (u < 0.0f || u > 1.0f) return;
  v3 qvec = cross(tvec, edge1);
  float v = dot(d, qvec) * inv_det;
  if (v < 0.0f || u + v > 1.0f) return;
  float t = dot(edge2, qvec) * inv_det;
  int islot = as_int(r0.w);
  bool closer = (t > 0 && t < best.t) || (t > 0 && t == best.t && best_i >= 0 && islot < best_i);
  if (closer) { best.t = t; best.set(3, slot_in_leaf_order); best.u = u; best.v = v; best_i = islot; }
}

// `lds_first` >= 0: the leaf's records are read from `lds_tris` (an LDS copy) starting at triangle lds_first instead of
// from the global array; the leaf-order slot reported for a hit is the global one either way.
template <bool COUNT>
__device__ __forceinline__ void test_leaf(const DevScene& S, int32_t leaf, v3 o, v3 d, HitRec& best, int& best_i, LocalCounters& lc,
                                          const float4* lds_tris = nullptr, int lds_first = -1) {
  uint32_t code = ~(uint32_t)leaf;
  uint32_t first = code >> 3, cnt = (code & 7u) + 1u;
  if (lds_first >= 0) {
    for (uint32_t k = 0; k < cnt; k += 2) {            // two records per round, both read before either is tested (a wall quad is one round)
      const bool two = k + 1 < cnt;
      const float4* ta = lds_tris + 3 * ((uint32_t)lds_first + k);
      const float4* tb = lds_tris + 3 * ((uint32_t)lds_first + k + (two ? 1u : 0u));
      float4 a0 = ta[0], a1 = ta[1], a2 = ta[2];
      float4 b0 = tb[0], b1 = tb[1], b2 = tb[2];
      test_triangle<COUNT>(a0, a1, a2, (int)(first + k), o, d, best, best_i, lc);
      if (two) test_triangle<COUNT>(b0, b1, b2, (int)(first + k + 1), o, d, best, best_i, lc);
    }
    return;
  }
  // two triangles per round: both records are requested before either is tested, so a leaf of 4 costs two memory
  // round trips on the dependent chain instead of four
  for (uint32_t k = 0; k < cnt; k += 2) {
    const float4* ta = (const float4*)((const char*)S.tri_verts + (first + k) * 48u);   // uniform base + 32-bit byte offset (< 4 GiB: checked on the host)
    bool two = k + 1 < cnt;
    const float4* tb = (const float4*)((const char*)S.tri_verts + (first + k + (two ? 1u : 0u)) * 48u);
    float4 a0 = ta[0], a1 = ta[1], a2 = ta[2];
    float4 b0 = tb[0], b1 = tb[1], b2 = tb[2];
    test_triangle<COUNT>(a0, a1, a2, (int)(first + k), o, d, best, best_i, lc);
    if (two) test_triangle<COUNT>(b0, b1, b2, (int)(first + k + 1), o, d, best, best_i, lc);
  }
}

// ---------------------------------------------------------------------------------------------------
// triangle BVH traversal for one MeshObject.  Replaces the brute-force loop RS:243-266 and returns
// the same winner: minimum t, ties inside one call going to the lowest index slot (A.4).
// Stack: LDS, entry e of this lane at stk[e * 64].  Cursor values: >= 0 interior node, < 0 leaf code,
// kBlasDone = traversal finished.
// ---------------------------------------------------------------------------------------------------
static constexpr int32_t kBlasDone = (int32_t)0x80000000;   // never a valid leaf code (it would be ~0x7fffffff)

// per-ray constants of the slab test on centre / half-extent boxes (include/urt_math.h "Slab test of the triangle BVH ..."): the
// traversal reads S.blas_cnodes, the (c, h) copy of the builders' [lo, hi] nodes —
//   q0 = c0.xyz, h0.x   q1 = h0.yz, c1.xy   q2 = c1.z, h1.xyz   q3 = child0, child1 (int bits), cone words of the two children (0 = none)
using BlasRay = CRay;
__device__ __forceinline__ BlasRay blas_ray(v3 o, v3 d) { return cray(o, d); }
// both children's [t near, t far]
__device__ __forceinline__ void cnode_slabs(float4 q0, float4 q1, float4 q2, const BlasRay& R, float tbest, float& tn0, float& tf0, float& tn1, float& tf1) {
  cslab(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, R, tbest, tn0, tf0);
  cslab(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, R, tbest, tn1, tf1);
}

__device__ __forceinline__ int32_t blas_pop(int* stk, int& sp) {
  if (sp == 0) return kBlasDone;
  sp--;
  return stk[sp * 64];
}

// One interior-node step: slab-test both children against [0, tbest], descend into the nearer hit child (ties: child 0),
// push the other; returns the next cursor.
__device__ __forceinline__ int32_t blas_node_eval(float4 q0, float4 q1, float4 q2, float4 q3, const BlasRay& R, float tbest, int* stk, int& sp) {
  float tn0, tf0, tn1, tf1;
  cnode_slabs(q0, q1, q2, R, tbest, tn0, tf0, tn1, tf1);
  bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
  int32_t c0 = as_int(q3.x), c1 = as_int(q3.y);
  if (h0 && h1) {
    bool swap = tn1 < tn0;
    stk[sp * 64] = swap ? c0 : c1;
    sp++;
    return swap ? c1 : c0;
  }
  if (h0) return c0;
  if (h1) return c1;
  return blas_pop(stk, sp);
}

// The same step without branches (the traversal loop of k_sched: per-wave instruction count is what bounds it, and the three-way
// branch of blas_node_eval costs a dozen scalar instructions per trip): the would-be pop value is read ahead (the LDS read
// overlaps the node fetch), the far child is written to the free slot above the stack top whether or not it is pushed (slot
// sp <= depth of the tree always exists: the stack has depth + 1 entries), and cursor / height are selected.
__device__ __forceinline__ int32_t blas_node_eval_flat(float4 q0, float4 q1, float4 q2, float4 q3, const BlasRay& R, float tbest, int* stk, int& sp) {
  int below = stk[max(sp - 1, 0) * 64];
  float tn0, tf0, tn1, tf1;
  cnode_slabs(q0, q1, q2, R, tbest, tn0, tf0, tn1, tf1);
  bool h0 = tn0 <= tf0, h1 = tn1 <= tf1;
  int32_t c0 = as_int(q3.x), c1 = as_int(q3.y);
  bool both = h0 && h1, none = !h0 && !h1;
  bool first1 = h1 && (!h0 || tn1 < tn0);          // child 1 is visited first: the only hit, or the nearer of two (ties: child 0)
  stk[sp * 64] = first1 ? c0 : c1;                  // the far child, where a push would put it
  int32_t popped = sp > 0 ? below : kBlasDone;
  int32_t nxt = none ? popped : (first1 ? c1 : c0);
  sp += both ? 1 : (none && sp > 0 ? -1 : 0);
  return nxt;
}

// The traversal loop of k_sched keeps the stack as a POINTER to its top entry (the one a pop returns) and a sentinel kBlasDone in
// entry 0 (written once per lane; a traversal starts at height 1): no address arithmetic per step (the far child goes to top[64], an
// immediate offset), no empty-stack test (popping the sentinel ends the traversal).  On this chip a compare, a select or a
// three-operand integer add each cost 1.8 fma (profiles/r03_logs/r3_valu_table_microbench.log): six of them per node step go.
__device__ __forceinline__ int32_t blas_node_select_ptr(bool h0, bool h1, float tn0, float tn1, int32_t c0, int32_t c1, int32_t below, int*& top_) {
  bool both = h0 && h1, none = !h0 && !h1;
  bool first1 = h1 && (!h0 || tn1 < tn0);          // child 1 is visited first: the only hit, or the nearer of two (ties: child 0)
  top_[64] = first1 ? c0 : c1;                      // the far child, where a push would put it
  int32_t nxt = none ? below : (first1 ? c1 : c0);
  top_ += both ? 64 : (none ? -64 : 0);
  return nxt;
}
__device__ __forceinline__ int32_t blas_node_eval_ptr(float4 q0, float4 q1, float4 q2, float4 q3, const BlasRay& R, float tbest, int*& top_) {
  int32_t below = *top_;
  float tn0, tf0, tn1, tf1;
  cnode_slabs(q0, q1, q2, R, tbest, tn0, tf0, tn1, tf1);
  return blas_node_select_ptr(tn0 <= tf0, tn1 <= tf1, tn0, tn1, as_int(q3.x), as_int(q3.y), below, top_);
}

// Normal cones (csrc/cones.hip, option "blas_cones"): q3.z / q3.w of a (c, h) node hold one dword per child, four signed bytes
// (ax, ay, az, T): every triangle below the child has its normal inside a cone about the axis a, and T is chosen so that
//     ax rx + ay ry + az rz - 127 T > 0,   r = round(127 d),
// implies d . (e1 x e2) >= 2^-16 |e1| |e2| for all of them (for | |d| - 1 | <= 2^-10; derivation in cones.hip): Moller-Trumbore's
// det = -d . (e1 x e2) is then negative, test_triangle rejects every one of them (det < kEPSILON), and the child need not be entered.
// Word 0 never skips (the test is strict): a child without a cone, and every child while the option is off.
// The ray's word: the three rounded components and -127, one register, derived once per phase entry.
__device__ __forceinline__ int cone_ray_word(v3 d) {
  int x = (int)__builtin_rintf(f_max(f_min(127.0f * d.x, 127.0f), -127.0f));      // (minNum / maxNum: a NaN component becomes a bound)
  int y = (int)__builtin_rintf(f_max(f_min(127.0f * d.y, 127.0f), -127.0f));
  int z = (int)__builtin_rintf(f_max(f_min(127.0f * d.z, 127.0f), -127.0f));
  return (x & 0xff) | ((y & 0xff) << 8) | ((z & 0xff) << 16) | (int)0x81000000u;
}
__device__ __forceinline__ bool cone_skips(float word, int rw) { return __builtin_amdgcn_sdot4(as_int(word), rw, 0, false) > 0; }
// blas_node_eval_ptr with the cone test: a child the ray sees from behind counts as missed
__device__ __forceinline__ int32_t blas_node_eval_cone_ptr(float4 q0, float4 q1, float4 q2, float4 q3, const BlasRay& R, float tbest, int rw, int*& top_) {
  int32_t below = *top_;
  float tn0, tf0, tn1, tf1;
  cnode_slabs(q0, q1, q2, R, tbest, tn0, tf0, tn1, tf1);
  bool h0 = tn0 <= tf0 && !cone_skips(q3.z, rw), h1 = tn1 <= tf1 && !cone_skips(q3.w, rw);
  return blas_node_select_ptr(h0, h1, tn0, tn1, as_int(q3.x), as_int(q3.y), below, top_);
}

// The same step on a 32-byte QUANTIZED node (csrc/qnodes.hip): two dwordx4 loads instead of four.  The twelve planes are 16-bit grid
// coordinates q; a plane's slab value is t = (origin + q cell - (o +- pad)) / d = fma(Q, S, B) with Q = 2^23 + q — built in ONE
// instruction per plane by putting q into the mantissa of 2^23 (0x4B000000 | q) —, S = cell / d and B = (origin - (o +- pad)) / d - 2^23 S
// per axis (QRay, derived from the ray at phase entry).  The 2^23 S terms cancel exactly but for the rounding of B: one cell at worst
// (|B| < 2^24 S), plus 2^-24 |origin| from the inner fma (<= 1/16 cell: the grid's cell is at least 2^-20 of it); the per-ray pad covers
// the rounding of o.  The two cells the quantizer adds on every face cover the rest (tests/test_qnodes_ref.py checks both on rays near
// box faces, grazing and axis-parallel ones included).  Conservative culling only: the hits are the triangle tests'.
struct QRay { v3 S, Bp, Bm; };
__device__ __forceinline__ QRay make_qray(v3 o, v3 d, float4 forg, float4 fcell) {
  // the quantized planes are [lo, hi] planes: their per-ray constants are -(o +- pad) / d
  const float pad = f_max(f_max(f_abs(o.x), f_abs(o.y)), f_abs(o.z)) * 1.52587890625e-5f;
  const v3 idir = mk3(blas_rcp(d.x), blas_rcp(d.y), blas_rcp(d.z));
  const v3 nop = mk3(-((o.x + pad) * idir.x), -((o.y + pad) * idir.y), -((o.z + pad) * idir.z));
  const v3 nom = mk3(-((o.x - pad) * idir.x), -((o.y - pad) * idir.y), -((o.z - pad) * idir.z));
  QRay Q;
  Q.S = mk3(fcell.x * idir.x, fcell.y * idir.y, fcell.z * idir.z);
  Q.Bp = mk3(f_fma(-8388608.0f, Q.S.x, f_fma(forg.x, idir.x, nop.x)), f_fma(-8388608.0f, Q.S.y, f_fma(forg.y, idir.y, nop.y)),
             f_fma(-8388608.0f, Q.S.z, f_fma(forg.z, idir.z, nop.z)));
  Q.Bm = mk3(f_fma(-8388608.0f, Q.S.x, f_fma(forg.x, idir.x, nom.x)), f_fma(-8388608.0f, Q.S.y, f_fma(forg.y, idir.y, nom.y)),
             f_fma(-8388608.0f, Q.S.z, f_fma(forg.z, idir.z, nom.z)));
  return Q;
}
__device__ __forceinline__ float q_lo16(float w) { return as_float((int)(((unsigned int)as_int(w) & 0xffffu) | 0x4B000000u)); }
__device__ __forceinline__ float q_hi16(float w) { return as_float((int)__builtin_amdgcn_alignbit(0x4B00u, (unsigned int)as_int(w), 16u)); }
__device__ __forceinline__ int32_t qnode_eval_ptr(float4 u0, float4 u1, const QRay& Q, float tbest, int*& top_) {
  int32_t below = *top_;
  // child 0: lo (u0.x lo16, u0.x hi16, u0.y lo16) hi (u0.y hi16, u0.z lo16, u0.z hi16); child 1: the same from u0.w, u1.x, u1.y
  float a1x = f_fma(q_lo16(u0.x), Q.S.x, Q.Bp.x), a2x = f_fma(q_hi16(u0.y), Q.S.x, Q.Bm.x);
  float a1y = f_fma(q_hi16(u0.x), Q.S.y, Q.Bp.y), a2y = f_fma(q_lo16(u0.z), Q.S.y, Q.Bm.y);
  float a1z = f_fma(q_lo16(u0.y), Q.S.z, Q.Bp.z), a2z = f_fma(q_hi16(u0.z), Q.S.z, Q.Bm.z);
  float tn0 = f_max(f_max(f_min(a1x, a2x), f_min(a1y, a2y)), f_max(f_min(a1z, a2z), 0.0f));
  float tf0 = f_min(f_min(f_max(a1x, a2x), f_max(a1y, a2y)), f_min(f_max(a1z, a2z), tbest));
  float b1x = f_fma(q_lo16(u0.w), Q.S.x, Q.Bp.x), b2x = f_fma(q_hi16(u1.x), Q.S.x, Q.Bm.x);
  float b1y = f_fma(q_hi16(u0.w), Q.S.y, Q.Bp.y), b2y = f_fma(q_lo16(u1.y), Q.S.y, Q.Bm.y);
  float b1z = f_fma(q_lo16(u1.x), Q.S.z, Q.Bp.z), b2z = f_fma(q_hi16(u1.y), Q.S.z, Q.Bm.z);
  float tn1 = f_max(f_max(f_min(b1x, b2x), f_min(b1y, b2y)), f_max(f_min(b1z, b2z), 0.0f));
  float tf1 = f_min(f_min(f_max(b1x, b2x), f_max(b1y, b2y)), f_min(f_max(b1z, b2z), tbest));
  return blas_node_select_ptr(tn0 <= tf0, tn1 <= tf1, tn0, tn1, as_int(u1.z), as_int(u1.w), below, top_);
}

// One interior-node step: slab-test both children against [0, tbest], descend into the nearer hit child (ties: child 0),
// push the other; returns the next cursor.
template <bool COUNT>
__device__ __forceinline__ int32_t blas_node_step(const DevScene& S, int32_t cur, const BlasRay& R, float tbest, int* stk, int& sp,
                                                  LocalCounters& lc) {
  if (COUNT) lc.blas_nodes++;
  // uniform base + 32-bit byte offset (the node array is < 4 GiB: checked on the host), so the load needs no 64-bit address math
  const float4* n = (const float4*)((const char*)S.blas_cnodes + ((uint32_t)cur << 6));
  float4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3];
  return blas_node_eval(q0, q1, q2, q3, R, tbest, stk, sp);
}

// The same step on a node of the LDS-resident top of the forest (nodes [0, top_nodes), 4 x float4 each)
template <bool COUNT>
__device__ __forceinline__ int32_t blas_node_step_top(const float4* top, int32_t cur, const BlasRay& R, float tbest, int* stk, int& sp,
                                                      LocalCounters& lc) {
  if (COUNT) lc.blas_nodes++;
  const float4* n = top + 4 * cur;
  return blas_node_eval_flat(n[0], n[1], n[2], n[3], R, tbest, stk, sp);
}

// The walk of the LDS-resident top with the stack in pointer form (entry 0 of `bl` holds the sentinel, heights start at 1: k_sched and
// k_serve): `sp` is the height before and after.  Six half-rate instructions fewer per step than the index form above.
// CONES: with the cone test (rw = cone_ray_word of the ray); never together with COUNT.
template <bool COUNT, bool CONES = false>
__device__ __forceinline__ int32_t blas_walk_top_ptr(const float4* top, int top_nodes, int32_t cur, const BlasRay& R, float tbest, int* bl, int& sp, LocalCounters& lc,
                                                     int rw = 0) {
  int* spp = bl + (sp - 1) * 64;
  do {
    if (COUNT) lc.blas_nodes++;
    const float4* n = top + 4 * cur;
    cur = CONES ? blas_node_eval_cone_ptr(n[0], n[1], n[2], n[3], R, tbest, rw, spp) : blas_node_eval_ptr(n[0], n[1], n[2], n[3], R, tbest, spp);
  } while (cur >= 0 && cur < top_nodes);
  sp = ((int)(spp - bl) >> 6) + 1;
  return cur;
}

template <bool COUNT>
__device__ __forceinline__ void intersect_mesh(const DevScene& S, int32_t root, v3 o, v3 d, HitRec& best,
                                               int* stk, LocalCounters& lc) {
  if (root == kEmptyMeshRoot) return;
  BlasRay R = blas_ray(o, d);
  int best_i = -1;          // index slot of a hit made in THIS call (enables the equal-t tie rule)
  int sp = 0;
  int32_t cur = root;
  while (cur != kBlasDone) {
    if (cur >= 0) {
      cur = blas_node_step<COUNT>(S, cur, R, best.t, stk, sp, lc);
    } else {
      test_leaf<COUNT>(S, cur, o, d, best, best_i, lc);
      cur = blas_pop(stk, sp);
    }
  }
}

// intersect_mesh with an early exit after the first leaf that produced a hit (any-hit form)
__device__ __forceinline__ void intersect_mesh_any(const DevScene& S, int32_t root, v3 o, v3 d, HitRec& best, int* stk, LocalCounters& lc) {
  if (root == kEmptyMeshRoot) return;
  BlasRay R = blas_ray(o, d);
  int best_i = -1;
  int sp = 0;
  int32_t cur = root;
  while (cur != kBlasDone) {
    if (cur >= 0) {
      cur = blas_node_step<false>(S, cur, R, best.t, stk, sp, lc);
    } else {
      test_leaf<false>(S, cur, o, d, best, best_i, lc);
      if (best.kid != 0) return;
      cur = blas_pop(stk, sp);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Trace — RS:364-383: ground plane, then the mesh object BVH, then the sphere BVH, for hits with 0 < t < t_max (t_max > 0, not NaN;
// +inf is the reference's Trace; kind 0 = nothing nearer than t_max).  ANY: return at the first such hit (ground plane, a leaf's
// triangles, a sphere).  tl / bl: this lane's LDS stacks for the object-level and the triangle-level traversals (lane_stacks).
// The ONE walk of a single ray: the frame kernels of modes 0 - 2, the ray queries, the feature buffers and the radiance queries call it.
// ---------------------------------------------------------------------------------------------------
template <bool COUNT, bool ANY>
__device__ __forceinline__ HitRec trace_ray(const DevScene& S, v3 o, v3 d, float t_max, int* tl, int* bl, LocalCounters& lc) {
  lc.rays++;
  HitRec best; best.t = t_max; best.kid = 0; best.u = 0; best.v = 0;
  float t_ground = URT_INF;                                     // what the object-level cull compares with (urt_math.h tlas_cull): the ground hit, whatever t_max
  // IntersectGroundPlane RS:156-172
  {
    float t = -o.y / d.y;
    if (t > 0 && t < URT_INF) t_ground = t;
    if (t > 0 && t < best.t) { best.t = t; best.kid = 1; }
    if (ANY && best.kid != 0) return best;
  }
  // one reciprocal per axis for the object-level slab test (normative form of RS:282-283)
  v3 rcp = mk3(1.0f / (d.x + kEPSILON), 1.0f / (d.y + kEPSILON), 1.0f / (d.z + kEPSILON));
  // IntersectMeshBVH RS:294-326 (`tests` is never reset: once a leaf was reached, every later popped
  // node has its object intersected, A.5; object ids < 0 or out of range are skipped, not read)
  if (S.n_meshes > 0) {
    int check = 1; tl[0] = 0; bool seen = false;
    while (check > 0) {
      check--;
      int bi = tl[check * 64];
      bool hit = false, culled = false; int index = -1;
      if (bi < S.n_mesh_tlas) {
        if (COUNT) lc.tlas_nodes++;
        float4 a = S.mesh_tlas[2 * bi], b = S.mesh_tlas[2 * bi + 1];
        index = as_int(a.w);
        float t_min, t_far;
        hit = tlas_slab_t(a, b, o, rcp, t_min, t_far);
        culled = leaf_culled(b, t_min, t_far, t_ground);
      }
      if (hit) {
        if (index < 0) { tl[check * 64] = bi * 2 + 1; check++; tl[check * 64] = bi * 2 + 2; check++; }
        else seen = true;
      }
      if (seen && !culled && index >= 0 && index < S.n_meshes) {
        if (ANY) {
          intersect_mesh_any(S, S.mesh_root[index], o, d, best, bl, lc);
          if (best.kid != 0) return best;
        } else {
          intersect_mesh<COUNT>(S, S.mesh_root[index], o, d, best, bl, lc);
        }
      }
    }
  }
  // IntersectSphereBVH RS:329-361
  if (S.n_spheres > 0) {
    int check = 1; tl[0] = 0; bool seen = false;
    while (check > 0) {
      check--;
      int bi = tl[check * 64];
      bool hit = false; int index = -1;
      if (bi < S.n_sphere_tlas) {
        if (COUNT) lc.tlas_nodes++;
        float4 a = S.sphere_tlas[2 * bi], b = S.sphere_tlas[2 * bi + 1];
        index = as_int(a.w);
        hit = tlas_slab(a, b, o, rcp);
      }
      if (hit) {
        if (index < 0) { tl[check * 64] = bi * 2 + 1; check++; tl[check * 64] = bi * 2 + 2; check++; }
        else seen = true;
      }
      if (seen && index >= 0 && index < S.n_spheres) {
        intersect_sphere<COUNT>(S, index, o, d, best, lc);
        if (ANY && best.kid != 0) return best;
      }
    }
  }
  return best;
}

// This lane's two stacks in the workgroup's dynamic LDS, laid out [entry][lane] per wave: tlas_stack + blas_stack entries per lane
__device__ __forceinline__ void lane_stacks(int tlas_stack, int blas_stack, int*& tl, int*& bl) {
  extern __shared__ int lds[];
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int per_wave = (tlas_stack + blas_stack) * 64;
  tl = lds + wave * per_wave + lane;
  bl = tl + tlas_stack * 64;
}

// A result is written once and not read again by its kernel: stored non-temporally so that it does not push BVH lines out of the L2
// (measured -1 % on the frame kernels; the same hint on the sky's texel loads costs +3 % and is not used).
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st_nt(float4* p, float4 v) {
  f4v q = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(q, (f4v*)p);
}

}  // namespace
