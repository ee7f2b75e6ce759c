// cones.h — normal cones of the triangle-BVH children, option "blas_cones" (see cones.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace urtd {

// The leaf-order triangle range below every child: int4 per node (first0, count0, first1, count1; first < 0: no range), found by
// max_depth relaxation sweeps between rng_a and rng_b (n_nodes int4 each); *out = the one that holds the result.  Once per scene: a refit
// keeps the topology.
hipError_t cone_ranges(const float4* nodes, int n_nodes, int max_depth, int4* rng_a, int4* rng_b, const int4** out, hipStream_t st);

// The cone word of every child from the world-space triangle records -> cnodes[4n + 3].z / .w (csrc/qnodes.hip k_center has written the
// rest of the node and zeros there) — after a build and after every refit.
hipError_t cone_words(const int4* rng, int n_nodes, const float4* tri_verts, int n_tris, float4* cnodes, hipStream_t st);

}  // namespace urtd
