// index_span.h — the span of vertices every MeshObject's index range refers to, found on the GPU (see index_span.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace urtd {

// Indices one work item (one wave) scans.  A MeshObject's scanned range is cut into pieces of this length from its own offset, so a piece
// boundary falls on every residue mod 3 of a long range (1024 = 3 * 341 + 1).
constexpr int kSpanChunk = 1024;

// One (MeshObject, chunk) pair: the wave scans _Indices[first .. first + count - 1] and joins the result into the MeshObject's two words.
struct SpanItem { int32_t mesh, first, count, pad; };

// The work table for the MeshObjects' (indices_offset, indices_count): each range is shortened to whole triangles and cut into chunks.
// A MeshObject with fewer than three indices gets no item.  False (and an empty table) when a range lies outside [0, n_indices): nothing
// may be launched then.
bool span_items(const int32_t* offsets, const int32_t* counts, int n_meshes, int n_indices, std::vector<SpanItem>& out);

// lo_hi[2 m] = the signed minimum, lo_hi[2 m + 1] = the signed maximum of the indices MeshObject m's items cover; INT32_MAX / -1 for a
// MeshObject without items.  Initialises lo_hi (2 * n_meshes words) and runs the items (a device copy of span_items' table), both on `st`.
// Every read lies inside an item's range.  Integer min / max: the result does not depend on the order the waves finish in.
hipError_t index_spans(const int32_t* indices, const SpanItem* items, int n_items, int32_t* lo_hi, int n_meshes, hipStream_t st);

}  // namespace urtd
