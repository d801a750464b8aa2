// Gradient clipping over spans of one flat gradient buffer (torch.nn.utils.clip_grad_norm_ / clip_grad_value_ semantics;
// factorized_amd.nn_utils).
//
// Unlike the optimizer spans a clip span ends anywhere: it is a tensor's exact extent, and the up to 63 floats of padding behind
// a tensor neither enter a norm nor change their bits.  SpanHead.e4 is the end rounded UP to a float4 and SpanHead.flags holds
// `end & 3`: when it is not 0 the span's last float4 has that many live lanes, which are loaded and stored one float at a time.
//
// The norm clip is two plain launches of the same grid.  The first leaves one partial per workgroup in `ws`; the second has
// EVERY workgroup add up all the partials in the same order -- so all of them hold the same bits of total_norm and of the
// coefficient -- and then scale its own tiles.  No atomics and nobody waits inside a launch: the result is a function of the
// span table alone, bit for bit.
#include <math.h>

#include "span_tiles.h"

namespace mfm {

constexpr int kClipMaxBlocks = 2048;      // the floats of `ws`: one partial per workgroup (span_grid deals at most 2048)

struct ClipSpanDev {
  SpanHead h;
};
// 112 x 16 bytes + 8
struct ClipSpansDev {
  ClipSpanDev s[MFM_CLIP_MAX_SPANS];
  int32_t count, tiles;
};
static_assert(sizeof(ClipSpansDev) + 4 * sizeof(void*) + 16 <= 4096, "clip span table exceeds the kernel argument limit");

// live lanes of the float4 at index i of a span: 4, or `end & 3` in the span's last float4
__device__ __forceinline__ int clip_lanes(const SpanHead& h, int64_t i) {
  return (h.flags != 0 && i == (int64_t)h.e4 - 1) ? h.flags : 4;
}

// the float4 at index i with its dead lanes (past the span's end) as 0.0f; those are not read
__device__ __forceinline__ f32x4 clip_load(const float* __restrict__ g, int64_t i, int lanes) {
  if (lanes == 4) return reinterpret_cast<const f32x4*>(g)[i];
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < lanes) v[j] = g[4 * i + j];
  return v;
}

// ... and its store: dead lanes are not written
__device__ __forceinline__ void clip_store(float* __restrict__ g, int64_t i, int lanes, f32x4 v) {
  if (lanes == 4) {
    reinterpret_cast<f32x4*>(g)[i] = v;
    return;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < lanes) g[4 * i + j] = v[j];
}

// the accumulation of one norm kind: sum of squares (L2), sum of |g| (L1), max of |g| (inf).  torch's max propagates a NaN,
// fmaxf drops it: the comparison is written out.
template <int KIND>
__device__ __forceinline__ float clip_acc(float a, float b) {
  if (KIND == MFM_NORM_INF) return (b > a || b != b) ? b : a;
  return a + b;
}

template <int KIND>
__device__ __forceinline__ float clip_term(float x) {
  return KIND == MFM_NORM_L2 ? x * x : fabsf(x);
}

// Reduce one value per thread over the workgroup (4 waves of 64): lanes by shuffles, the 4 wave results through LDS, always in
// the same order.  Every thread returns the result.
template <int KIND>
__device__ __forceinline__ float clip_block_reduce(float v, float* lds) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = clip_acc<KIND>(v, __shfl_down(v, off, 64));
  __syncthreads();                         // (lds may still be read from the call before)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = lds[0];
#pragma unroll
  for (int w = 1; w < kSpanTile / 64; ++w) r = clip_acc<KIND>(r, lds[w]);
  return r;
}

// Launch 1: ws[blockIdx.x] = this workgroup's partial over its tiles.
template <int KIND>
__global__ __launch_bounds__(kSpanTile) void clip_partials_kernel(const float* __restrict__ g, const ClipSpansDev S,
                                                                  float* __restrict__ ws) {
  __shared__ float lds[kSpanTile / 64];
  float acc = 0.0f;
  int k = 0;
  for (int t = blockIdx.x; t < S.tiles; t += gridDim.x) {
    k = span_of_tile(S, t, k);
    const SpanHead h = S.s[k].h;
    const int64_t i = span_tile_index(h, t);
    if (i >= h.e4) continue;
    const f32x4 v = clip_load(g, i, clip_lanes(h, i));
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = clip_acc<KIND>(acc, clip_term<KIND>(v[j]));
  }
  acc = clip_block_reduce<KIND>(acc, lds);
  if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

// Launch 2 (same grid): total_norm from all partials, then g *= min(max_norm / (total_norm + 1e-6), 1) over this workgroup's
// tiles.  The multiplication is unconditional, as torch's is: inf * 0 and NaN come out as they do there.
template <int KIND>
__global__ __launch_bounds__(kSpanTile) void clip_scale_kernel(float* __restrict__ g, const ClipSpansDev S,
                                                               const float* __restrict__ ws, float max_norm,
                                                               float* __restrict__ total_norm, const float* __restrict__ guard) {
  __shared__ float lds[kSpanTile / 64];
  // guard word (mfm_adam_flat_guarded): gradients that cannot be trusted are not rescaled and have no finite norm
  if (guard_raised(guard)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) total_norm[0] = NAN;
    return;
  }
  float acc = 0.0f;
  for (int b = threadIdx.x; b < (int)gridDim.x; b += kSpanTile) acc = clip_acc<KIND>(acc, ws[b]);
  acc = clip_block_reduce<KIND>(acc, lds);
  const float total = KIND == MFM_NORM_L2 ? sqrtf(acc) : acc;
  const float c = max_norm / (total + 1e-6f);
  const float coef = c > 1.0f ? 1.0f : c;          // (a NaN stays a NaN: torch.clamp(max=1.0))
  if (blockIdx.x == 0 && threadIdx.x == 0) total_norm[0] = total;
  int k = 0;
  for (int t = blockIdx.x; t < S.tiles; t += gridDim.x) {
    k = span_of_tile(S, t, k);
    const SpanHead h = S.s[k].h;
    const int64_t i = span_tile_index(h, t);
    if (i >= h.e4) continue;
    const int lanes = clip_lanes(h, i);
    f32x4 v = clip_load(g, i, lanes);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= coef;
    clip_store(g, i, lanes, v);
  }
}

// g = clamp(g, -c, c); a NaN stays a NaN (torch.clamp), so no fminf / fmaxf
__global__ __launch_bounds__(kSpanTile) void clip_value_kernel(float* __restrict__ g, const ClipSpansDev S, float c,
                                                               const float* __restrict__ guard) {
  if (guard_raised(guard)) return;
  int k = 0;
  for (int t = blockIdx.x; t < S.tiles; t += gridDim.x) {
    k = span_of_tile(S, t, k);
    const SpanHead h = S.s[k].h;
    const int64_t i = span_tile_index(h, t);
    if (i >= h.e4) continue;
    const int lanes = clip_lanes(h, i);
    f32x4 v = clip_load(g, i, lanes);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] > c ? c : (v[j] < -c ? -c : v[j]);
    clip_store(g, i, lanes, v);
  }
}

// Host: the checked table of a launch and its grid.  `who` starts every message.
static int clip_table(const char* who, const float* g, const MfmClipSpan* spans, int nspans, ClipSpansDev* S, int* nb) {
  MFM_REQUIRE(g && spans && nspans >= 1 && nspans <= MFM_CLIP_MAX_SPANS, "%s: bad arguments (nspans=%d, at most %d)", who, nspans,
              MFM_CLIP_MAX_SPANS);
  MFM_REQUIRE(((uintptr_t)g & 15) == 0, "%s: the gradient buffer must be 16-byte aligned", who);
  memset(S, 0, sizeof(*S));
  S->count = nspans;
  int64_t tiles = 0, prev_end = 0;
  for (int k = 0; k < nspans; ++k) {
    const int64_t begin = spans[k].begin, end = spans[k].end;
    // (begin is a multiple of 4 and not below the end before it: the float4s of two spans never overlap)
    MFM_REQUIRE(begin >= prev_end && end > begin && (begin & 3) == 0 && ((end + 3) >> 2) <= INT32_MAX,
                "%s[%d]: [%lld,%lld) (ascending, disjoint, begin a multiple of 4 elements)", who, k, (long long)begin,
                (long long)end);
    SpanHead& h = S->s[k].h;
    h.b4 = (int32_t)(begin >> 2);
    h.e4 = (int32_t)((end + 3) >> 2);
    h.tile0 = (int32_t)tiles;
    h.flags = (int32_t)(end & 3);
    tiles += (h.e4 - h.b4 + kSpanTile - 1) / kSpanTile;
    prev_end = end;
  }
  return span_grid(who, tiles, &S->tiles, nb);
}

int clip_norm_launch(float* g, const MfmClipSpan* spans, int nspans, int norm_kind, float max_norm, float* ws, float* total_norm,
                     const float* guard, hipStream_t stream) {
  static const char* who = "clip grad norm spans";
  MFM_REQUIRE(ws && total_norm, "%s: bad arguments (ws and total_norm must not be null)", who);
  MFM_REQUIRE(norm_kind == MFM_NORM_L2 || norm_kind == MFM_NORM_INF || norm_kind == MFM_NORM_L1, "%s: unknown norm_kind %d", who,
              norm_kind);
  MFM_REQUIRE(max_norm >= 0.0f, "%s: max_norm %g (must be >= 0, not NaN)", who, (double)max_norm);
  ClipSpansDev S;
  int nb;
  if (int rc = clip_table(who, g, spans, nspans, &S, &nb)) return rc;
  MFM_REQUIRE(nb <= kClipMaxBlocks, "%s: %d workgroups for a workspace of %d partials", who, nb, kClipMaxBlocks);
  const dim3 grid(nb), block(kSpanTile);
  switch (norm_kind) {
    case MFM_NORM_L2:
      MFM_LAUNCH_TIMED(clip_partials_kernel<MFM_NORM_L2>, grid, block, 0, stream, g, S, ws);
      MFM_LAUNCH_TIMED(clip_scale_kernel<MFM_NORM_L2>, grid, block, 0, stream, g, S, ws, max_norm, total_norm, guard);
      break;
    case MFM_NORM_INF:
      MFM_LAUNCH_TIMED(clip_partials_kernel<MFM_NORM_INF>, grid, block, 0, stream, g, S, ws);
      MFM_LAUNCH_TIMED(clip_scale_kernel<MFM_NORM_INF>, grid, block, 0, stream, g, S, ws, max_norm, total_norm, guard);
      break;
    default:
      MFM_LAUNCH_TIMED(clip_partials_kernel<MFM_NORM_L1>, grid, block, 0, stream, g, S, ws);
      MFM_LAUNCH_TIMED(clip_scale_kernel<MFM_NORM_L1>, grid, block, 0, stream, g, S, ws, max_norm, total_norm, guard);
      break;
  }
  MFM_LAUNCH_CHECK("clip_partials_kernel / clip_scale_kernel");
  return MFM_OK;
}

int clip_value_launch(float* g, const MfmClipSpan* spans, int nspans, float clip_value, const float* guard, hipStream_t stream) {
  static const char* who = "clip grad value spans";
  MFM_REQUIRE(clip_value >= 0.0f, "%s: clip_value %g (must be >= 0, not NaN)", who, (double)clip_value);
  ClipSpansDev S;
  int nb;
  if (int rc = clip_table(who, g, spans, nspans, &S, &nb)) return rc;
  MFM_LAUNCH_TIMED(clip_value_kernel, dim3(nb), dim3(kSpanTile), 0, stream, g, S, clip_value, guard);
  MFM_LAUNCH_CHECK("clip_value_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_clip_workspace_floats(void) { return mfm::kClipMaxBlocks; }

extern "C" int mfm_clip_grad_norm_flat_spans(float* g, const MfmClipSpan* spans, int32_t nspans, int32_t norm_kind, float max_norm,
                                             float* ws, float* total_norm, const float* guard, void* stream) {
  return mfm::clip_norm_launch(g, spans, nspans, norm_kind, max_norm, ws, total_norm, guard, (hipStream_t)stream);
}

extern "C" int mfm_clip_grad_value_flat_spans(float* g, const MfmClipSpan* spans, int32_t nspans, float clip_value,
                                              const float* guard, void* stream) {
  return mfm::clip_value_launch(g, spans, nspans, clip_value, guard, (hipStream_t)stream);
}
