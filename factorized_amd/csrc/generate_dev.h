// What the inference launches built on small_fwd_body<.., REC = false> share (generate.hip, impute.hip): the rows of a factor
// into LDS, and the host's sizing rules -- chunk rows, tile rows, the LDS the recurrence lays out.
#pragma once
#include <algorithm>

#include "lstm_seq_small_dev.h"
#include "dense_rows_dev.h"

namespace mfm {

// rows [b0, b0 + R) of z [n, zs] -> LDS [zs][R]; rows beyond n: zeros
template <int R>
__device__ __forceinline__ void stage_rows(const float* __restrict__ z, const int zs, const int b0, const int n, float* out) {
  for (int e = threadIdx.x; e < zs * R; e += blockDim.x) {
    const int r = e / zs, k = e - r * zs;
    out[k * R + r] = (b0 + r < n) ? z[(int64_t)(b0 + r) * zs + k] : 0.0f;
  }
  lds_barrier();
}

// ---------------------------------------------------------------- host
static int64_t gen_rows(int64_t N, int64_t max_rows) { return (max_rows > 0 && max_rows < N) ? max_rows : N; }
static int64_t hp_of(int64_t h) { return (h + 15) / 16 * 16; }

// floats of LDS small_fwd_body<KQ, R> lays out for hidden size h (its two h buffers, then the weight staging panel / its record
// and x-projection buffers, layout kept), a multiple of 4
static size_t seq_lds_floats(int h, int R) {
  const size_t HKB = (size_t)round_up(4 * round_up(cdiv(h, 4), 2), 16);
  const size_t hh = (R == 1 && (h & 3) == 0) ? 0 : (size_t)h * h;
  const size_t rec = (2 * 6 + 2 * 4) * HKB * R;
  return (2 * HKB * R + std::max(2 * hh, rec) + 3) / 4 * 4;
}

static int gen_hk4(int h) { return round_up(cdiv(h, 4), 2); }

// one-row tiles below 6 workgroups per CU over the whole launch (the rule of the training recurrences), else four-row tiles
static int gen_tile_rows(int lstms, int rows) { return ((long)lstms * rows < 6L * device_cus()) ? 1 : 4; }

}  // namespace mfm
