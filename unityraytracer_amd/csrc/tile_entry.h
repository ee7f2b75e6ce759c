// tile_entry.h — the per-tile entry lists of the triangle BVH for camera rays (csrc/tile_entry.hip builds them on the GPU, k_sched's
// plain single-mesh FRONT starts its camera rays at them): the decision logic alone.  No HIP in here: the pre-pass kernel and a
// stand-alone host program (tests/tile_entry_main.cpp) run the same functions.
//
// While an image accumulates the camera is fixed and the frames of a launch differ only in their sub-pixel jitter, yet every camera ray
// of an 8x8 tile walks the BVH from the root through the same ancestors, at which the tile as a whole provably never enters the sibling.
// tile_entry_list walks that common part once per tile: from the mesh's root it keeps a frontier of at most kTileEntryK nodes and
// refines the shallowest one — replaces it by those of its children that some ray of the tile could enter — until the budget or the
// stack bound is reached.  A camera ray then starts with the frontier on its stack instead of the root.
//
// A child is DROPPED only when
//  (a) its box, inflated, lies wholly outside one side plane of the tile's frustum, or
//  (b) its cone word (csrc/cones.hip) makes trace_device.h cone_skips true for every ray of the tile.
//
// The tile's rays.  Pixel px of tile tx has its sample at s = px + rand + _PixelOffset.x with rand in [0, 1) and the offset in [0, 1]
// (the launch checks it): s in [8 tx, 8 tx + 9].  The rectangle is widened by one pixel on every side: [8 tx - 1, 8 tx + 10], the same
// in y.  The unnormalised direction of camera_ray_uv is affine in the sample position, so every ray of the tile is a non-negative
// combination of the four corner directions, computed here with camera_ray_uv's arithmetic.  The rounding of that arithmetic moves a direction
// by ~1e-6 rad; the pixel of widening is >= 3e-5 rad even on an image 65535 pixels high.  All rays of the frame leave from one origin,
// bit for bit (frame_derived.h), which is the apex of the frustum.
//
// (a) The plane test.  Side plane k passes through the origin and the corners k, k + 1 (unit vectors); its inward normal is
// n = +-cross(c_k, c_k+1), each component off by <= 2^-22 absolute.  A box (c, h) is outside when
//     n . (c - o) + |n| . h' < -E,     h' = h + pad,   pad = 2^-15 max|o| + 2^-20 (max|c| + max h),   E = 2^-19 (|c|_1 + |o|_1 + |h'|_1).
// pad: a triangle that Moller-Trumbore accepts for a ray lies, in real arithmetic, within the test's rounding of the ray, and the per-ray
// pad of urt_math.h cray (2^-16 max|o|) together with the build pad — which the box already contains — covers that rounding 64 times
// over; so the real ray passes through the box widened by 2^-16 max|o|, and twice that is used.  E: the error of the normal (2^-22 per
// component, times the L1 size of c - o and h') and of the evaluation (2^-24 per operation on terms of at most that size), 8 times over.
// A ray inside the frustum that passes through the widened box puts a point of that box on the inner side of every plane: not dropped.
//
// (b) The cone test.  The child's word is (ax, ay, az, T); a ray with bytes r = round(127 d) skips it iff a . r - 127 T > 0.  With
// d = sum w_k c_k / |sum w_k c_k|, w_k >= 0 and |sum w_k c_k| <= sum w_k:  a . d >= min_k a . c_k  WHEN that minimum is not negative,
// and a . r >= 127 a . d - 0.5001 |a|_1.  So  127 min_k a . c_k - |a|_1 > 127 T  (m >= 0) implies the skip for every ray of the tile;
// the second half of |a|_1 pays for | |d| - 1 | and the float evaluation of the left side (< 0.01).  Word 0 never drops.
//
// The stack.  A lane's traversal stack has one entry per level of the deepest leaf, plus the sentinel and the slot above the top
// (scene_prep.cpp: blas_stack = max depth + 2).  A walk that starts below an entry of depth e with the other n - 1 entries under it needs
// (n - 1) + (max depth - e) + 2 entries at most: the frontier keeps  n - 1 <= depth of its shallowest entry, by refusing the refinement
// that would break it.
#pragma once
#include <stdint.h>

#include "../../include/urt_math.h"

namespace urtd {

static constexpr int kTileEntryK = 8;                           // entries per tile: 32 B
static constexpr int kTileEntryMaxK = 16;                       // what tile_entry_list can be asked for
static constexpr int kTileEntrySteps = 96;                      // node evaluations per tile at most
static constexpr int32_t kTileEntryDone = (int32_t)0x80000000;  // padding: trace_device.h kBlasDone

struct TileFrustum {
  urt::v3 o;          // apex: the frame's ray origin
  urt::v3 c[4];       // unit corner directions (x0,y0) (x1,y0) (x1,y1) (x0,y1) of the widened sample rectangle
  urt::v3 n[4];       // inward normal of the side plane through corners k, k + 1
  urt::v3 mid;        // the sum of the corners: orders the entries
  bool ok;            // false: degenerate (a zero or non-finite direction, planes that do not form a cone)
};

// one corner: camera_ray_uv's arithmetic (csrc/camera_device.h) at sample position (sx, sy) in pixels
URT_HD urt::v3 tile_corner_dir(const float* c2w, const float* invp, float sx, float sy, int width, int height) {
  float u = sx / (float)width * 2.0f - 1.0f;
  float v = sy / (float)height * 2.0f - 1.0f;
  urt::v3 dir = urt::mul_m4(invp, u, v, 0.0f, 1.0f);
  dir = urt::mul_m4(c2w, dir.x, dir.y, dir.z, 0.0f);
  return urt::normalize(dir);
}

URT_HD TileFrustum tile_frustum(const float* c2w, const float* invp, int tx, int ty, int width, int height) {
  TileFrustum F;
  F.o = urt::mul_m4(c2w, 0.0f, 0.0f, 0.0f, 1.0f);
  const float x0 = (float)(8 * tx - 1), x1 = (float)(8 * tx + 10), y0 = (float)(8 * ty - 1), y1 = (float)(8 * ty + 10);
  F.c[0] = tile_corner_dir(c2w, invp, x0, y0, width, height);
  F.c[1] = tile_corner_dir(c2w, invp, x1, y0, width, height);
  F.c[2] = tile_corner_dir(c2w, invp, x1, y1, width, height);
  F.c[3] = tile_corner_dir(c2w, invp, x0, y1, width, height);
  F.mid = (F.c[0] + F.c[1]) + (F.c[2] + F.c[3]);
  bool ok = true;
  for (int k = 0; k < 4; k++) {
    const urt::v3 a = F.c[k], b = F.c[(k + 1) & 3], opp = F.c[(k + 2) & 3], opp2 = F.c[(k + 3) & 3];
    ok = ok && urt::f_abs(a.x) <= 2.0f && urt::f_abs(a.y) <= 2.0f && urt::f_abs(a.z) <= 2.0f;      // (false for NaN / inf)
    urt::v3 n = urt::cross(a, b);
    float s = urt::dot(n, opp), s2 = urt::dot(n, opp2);
    if (s < 0.0f) { n = -n; s = -s; s2 = -s2; }
    // both other corners clearly on the inner side: the four planes bound a convex cone around the rays (1e-9: |n| >= 1e-4 and the
    // opposite corners >= 1e-4 rad away on any image this library accepts, so a real frustum gives >= 1e-8)
    ok = ok && s > 1e-9f && s2 > 1e-9f;
    F.n[k] = n;
  }
  const float o1 = urt::f_abs(F.o.x) + urt::f_abs(F.o.y) + urt::f_abs(F.o.z);
  F.ok = ok && o1 <= 1e30f && urt::dot(F.mid, F.mid) > 1.0f;     // (four unit vectors in a narrow cone sum to ~4)
  return F;
}

// (a): the box (c, h) of a (centre, half extent) node, inflated, lies wholly outside one side plane
URT_HD bool tile_box_outside(const TileFrustum& F, float cx, float cy, float cz, float hx, float hy, float hz) {
  if (!(hx >= 0.0f && hy >= 0.0f && hz >= 0.0f)) return hx < 0.0f && hy < 0.0f && hz < 0.0f;    // an empty box (urt_math.h box_center_form) is entered by no ray; NaN: kept
  const float omax = urt::f_max(urt::f_max(urt::f_abs(F.o.x), urt::f_abs(F.o.y)), urt::f_abs(F.o.z));
  const float cmax = urt::f_max(urt::f_max(urt::f_abs(cx), urt::f_abs(cy)), urt::f_abs(cz));
  const float hmax = urt::f_max(urt::f_max(hx, hy), hz);
  const float pad = 3.0517578125e-5f * omax + 9.5367431640625e-7f * (cmax + hmax);
  const float px = hx + pad, py = hy + pad, pz = hz + pad;
  const float rx = cx - F.o.x, ry = cy - F.o.y, rz = cz - F.o.z;
  const float size = (urt::f_abs(cx) + urt::f_abs(cy) + urt::f_abs(cz)) + (urt::f_abs(F.o.x) + urt::f_abs(F.o.y) + urt::f_abs(F.o.z)) + (px + py + pz);
  const float E = 1.9073486328125e-6f * size;
  bool out = false;
  for (int k = 0; k < 4; k++) {
    const urt::v3 n = F.n[k];
    const float far = (n.x * rx + n.y * ry + n.z * rz) + (urt::f_abs(n.x) * px + urt::f_abs(n.y) * py + urt::f_abs(n.z) * pz);
    out = out || far < -E;                                      // (NaN compares false: kept)
  }
  return out;
}

// (b): the cone word makes cone_skips true for every ray of the tile
URT_HD bool tile_cone_drops(const TileFrustum& F, uint32_t word) {
  if (word == 0u) return false;
  const float ax = (float)(int8_t)(word & 0xffu), ay = (float)(int8_t)((word >> 8) & 0xffu), az = (float)(int8_t)((word >> 16) & 0xffu);
  const float T = (float)(int8_t)(word >> 24);
  float m = 3.0e38f;
  for (int k = 0; k < 4; k++) m = urt::f_min(m, 127.0f * (ax * F.c[k].x + ay * F.c[k].y + az * F.c[k].z));
  if (!(m >= 0.0f)) return false;
  return m - (urt::f_abs(ax) + urt::f_abs(ay) + urt::f_abs(az)) > 127.0f * T;
}

// The entry list of one tile: out[0 .. K) = the frontier, nearest first, padded with kTileEntryDone; returns its length (0: no ray of the
// tile can hit the mesh).  cnodes: the (centre, half extent) nodes the trace kernels read (16 floats each, urt_math.h); n_nodes: their
// number; root: the mesh's root code (>= 0 an interior node; a leaf code or an empty mesh is returned as the list {root}).
URT_HD int tile_entry_list(const float* cnodes, int n_nodes, int32_t root, const TileFrustum& F, int K, int32_t* out) {
  int32_t node[kTileEntryMaxK]; int depth[kTileEntryMaxK]; float key[kTileEntryMaxK]; bool closed[kTileEntryMaxK];
  if (K > kTileEntryMaxK) K = kTileEntryMaxK;
  if (K < 1) K = 1;
  int n = 1;
  node[0] = root; depth[0] = 0; key[0] = 0.0f; closed[0] = !F.ok;
  for (int step = 0; step < kTileEntrySteps; step++) {
    int j = -1;
    for (int i = 0; i < n; i++)
      if (!closed[i] && node[i] >= 0 && node[i] < n_nodes && (j < 0 || depth[i] < depth[j])) j = i;
    if (j < 0) break;
    const float* q = cnodes + 16 * (size_t)node[j];
    // q0 = c0.xyz, h0.x   q1 = h0.yz, c1.xy   q2 = c1.z, h1.xyz   q3 = child0, child1, cone words (trace_device.h)
    const float bx[2][6] = {{q[0], q[1], q[2], q[3], q[4], q[5]}, {q[6], q[7], q[8], q[9], q[10], q[11]}};
    int32_t kid[2]; float kkey[2]; int ns = 0;
    for (int c = 0; c < 2; c++) {
      const int32_t child = (int32_t)urt::f_bits(q[12 + c]);
      const uint32_t word = urt::f_bits(q[14 + c]);
      if (child == kTileEntryDone) continue;                    // (never written by a builder; it would end a traversal)
      if (tile_box_outside(F, bx[c][0], bx[c][1], bx[c][2], bx[c][3], bx[c][4], bx[c][5]) || tile_cone_drops(F, word)) continue;
      kid[ns] = child;
      kkey[ns] = (bx[c][0] - F.o.x) * F.mid.x + (bx[c][1] - F.o.y) * F.mid.y + (bx[c][2] - F.o.z) * F.mid.z;
      ns++;
    }
    if (ns == 2) {                                              // the frontier grows by one: the budget, then the stack bound
      int dmin = depth[j] + 1;
      for (int i = 0; i < n; i++) if (i != j && depth[i] < dmin) dmin = depth[i];
      if (n + 1 > K || n > dmin) { closed[j] = true; continue; }
    }
    const int dj = depth[j] + 1;
    if (ns == 0) { n--; node[j] = node[n]; depth[j] = depth[n]; key[j] = key[n]; closed[j] = closed[n]; continue; }
    node[j] = kid[0]; depth[j] = dj; key[j] = kkey[0]; closed[j] = false;
    if (ns == 2) { node[n] = kid[1]; depth[n] = dj; key[n] = kkey[1]; closed[n] = false; n++; }
  }
  for (int i = 1; i < n; i++) {                                 // nearest first (insertion sort; NaN keys stay where they are)
    const int32_t nd = node[i]; const float ky = key[i];
    int p = i;
    while (p > 0 && key[p - 1] > ky) { node[p] = node[p - 1]; key[p] = key[p - 1]; p--; }
    node[p] = nd; key[p] = ky;
  }
  for (int i = 0; i < K; i++) out[i] = i < n ? node[i] : kTileEntryDone;
  return n;
}

// The table's record of a list of n entries e[0 .. n): word 0 = the first node a ray visits, words 1 .. K-1 = the lane's stack above the
// sentinel, bottom first — e[n-1] .. e[1] — and padding.  The ray pops e[1] next.
URT_HD void tile_entry_record(const int32_t* e, int n, int K, int32_t* rec) {
  rec[0] = n > 0 ? e[0] : kTileEntryDone;
  for (int i = 1; i < K; i++) rec[i] = i < n ? e[n - i] : kTileEntryDone;
}

}  // namespace urtd
