// Spans of one flat buffer dealt to workgroups in tiles: what the span kernels of sgd.hip and adam_ext.hip share.
//
// A launch carries a table `{Span s[N]; int32_t count, tiles;}` in its argument block; every Span begins with a SpanHead.  Work
// is dealt in tiles of 256 float4: span k owns tiles [tile0_k, tile0_{k+1}).  A workgroup walks its tiles in ascending order
// (grid-stride), so the span of the next tile is found by advancing k -- once per tile, uniform over the workgroup; the element
// loop holds no span search and every hyper-parameter branch is uniform.
#pragma once
#include "internal.h"

namespace mfm {

constexpr int kSpanTile = 256;      // float4 per tile = threads per workgroup

// bounds in float4 units, the first tile of the span in the launch's tile numbering, the optimizer's flags
struct SpanHead {
  int32_t b4, e4, tile0, flags;
};

// Host: span k of a launch covers elements [begin, end).  Checks the bounds against the end of the span before it, fills
// b4 / e4 / tile0 and moves *prev_end and *tiles on.  `who` starts every message ("sgd spans", "adam ext spans").
inline int span_head_fill(const char* who, int k, int64_t begin, int64_t end, int64_t* prev_end, int64_t* tiles, SpanHead* h) {
  MFM_REQUIRE(begin >= *prev_end && end > begin && (begin & 3) == 0 && (end & 3) == 0 && (end >> 2) <= INT32_MAX,
              "%s[%d]: [%lld,%lld) (ascending, disjoint, bounds multiples of 4 elements)", who, k, (long long)begin,
              (long long)end);
  h->b4 = (int32_t)(begin >> 2);
  h->e4 = (int32_t)(end >> 2);
  h->tile0 = (int32_t)*tiles;
  *tiles += (h->e4 - h->b4 + kSpanTile - 1) / kSpanTile;
  *prev_end = end;
  return MFM_OK;
}

// Host: the table's tile count and the grid of the launch (at most 2048 workgroups, grid-stride over the tiles).
inline int span_grid(const char* who, int64_t tiles, int32_t* table_tiles, int* nb) {
  MFM_REQUIRE(tiles <= INT32_MAX, "%s: %lld tiles", who, (long long)tiles);
  *table_tiles = (int32_t)tiles;
  *nb = (int)(tiles < 2048 ? tiles : 2048);
  return MFM_OK;
}

// Device: the span of tile t, searched upwards from span k (the span of the workgroup's tile before: tiles come ascending).
template <class Table>
__device__ __forceinline__ int span_of_tile(const Table& S, int t, int k) {
  while (k + 1 < S.count && t >= S.s[k + 1].h.tile0) ++k;
  return k;
}

// Device: this thread's float4 index in tile t of the span; the caller skips the element when the index is not below e4 (the
// last tile of a span may be partial).
__device__ __forceinline__ int64_t span_tile_index(const SpanHead& h, int t) {
  return (int64_t)h.b4 + (int64_t)(t - h.tile0) * kSpanTile + threadIdx.x;
}

}  // namespace mfm
