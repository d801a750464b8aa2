// Running average of one flat parameter buffer into another of the same layout (torch.optim.swa_utils.AveragedModel
// semantics; factorized_amd.swa_utils): avg = p on the first update, avg = lerp(avg, p, w) on every later one, over ONE
// contiguous range, and the update count advanced by the launch itself.
//
// The count n is the int64 word of AveragedModel.n_averaged in device memory: no host value takes part, so a captured launch
// does the right thing on every replay.  Every workgroup reads n before its first tile.  Behind its last tile it draws an
// arrival ticket (one agent-scope atomicAdd on an int32 word that is 0 between launches); the workgroup that draws
// gridDim.x - 1 knows that every workgroup has read n, stores n + 1 from one lane and puts the ticket word back to 0.  Nobody
// waits or spins: this is a ticket, not a barrier, and a 1-workgroup launch takes the same code.
//
// Why no workgroup can see n + 1 too early: a wave that has a tile uses n (the branch, SWA's weight) before its first store,
// so its load has returned before the workgroup's __syncthreads(); a wave without a tile computes nothing from n; lane 0's
// own load is ordered before its ticket by the release half of the atomicAdd, and the last arriver's store of n + 1 behind
// every earlier ticket by the acquire half.
//
// Work is dealt as in the other flat kernels (span_tiles.h): 256 threads, one float4 per thread and tile, at most 2048
// workgroups grid-striding over the tiles, 128-bit loads and stores, no LDS.  12 bytes of traffic per element.
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage):
//   avg_flat_kernel   VGPRs 20   AGPRs 0   SGPRs 30   scratch 0 bytes   LDS 0 bytes   occupancy 8 waves/SIMD
// In the generated code every wave waits for its load of n (s_waitcnt vmcnt(0)) before the first branch, the tiles move as
// global_load / global_store_dwordx4, 1 / (n + 1) is the IEEE division sequence, and n + 1 and the ticket's 0 leave as vector
// stores (sc1) from one lane.
#include <math.h>

#include "span_tiles.h"

namespace mfm {

enum { kAvgCopy = 0, kAvgLerpLow = 1, kAvgLerpHigh = 2 };

// This workgroup's tiles of float4s [b4, e4) in one of the three forms; the form is uniform over the launch.
template <int MODE>
__device__ __forceinline__ void avg_tiles(float* avg, const float* p, int64_t b4, int64_t e4, int tiles, float w) {
  const float omw = 1.0f - w;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = b4 + (int64_t)t * kSpanTile + threadIdx.x;
    if (i >= e4) continue;
    const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    if (MODE == kAvgCopy) {
      reinterpret_cast<f32x4*>(avg)[i] = pv;          // bit for bit: no arithmetic touches a NaN payload
      continue;
    }
    f32x4 av = reinterpret_cast<const f32x4*>(avg)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = pv[j] - av[j];
      av[j] = MODE == kAvgLerpLow ? av[j] + w * d : pv[j] - d * omw;      // torch's lerp (|w| < 0.5 or not)
    }
    reinterpret_cast<f32x4*>(avg)[i] = av;
  }
}

__global__ __launch_bounds__(kSpanTile) void avg_flat_kernel(float* avg, const float* p, int64_t b4, int64_t e4, int tiles,
                                                             int kind, float w_ema, int64_t* n_averaged, int32_t* ticket) {
  const int64_t n = __hip_atomic_load(n_averaged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n == 0) {
    avg_tiles<kAvgCopy>(avg, p, b4, e4, tiles, 0.0f);
  } else {
    // SWA: 1 / (n + 1) as torch forms it from the int64 tensor (to fp32, then an IEEE division)
    const float w = kind == MFM_AVG_SWA ? 1.0f / (float)(n + 1) : w_ema;
    if (fabsf(w) < 0.5f) avg_tiles<kAvgLerpLow>(avg, p, b4, e4, tiles, w);
    else avg_tiles<kAvgLerpHigh>(avg, p, b4, e4, tiles, w);
  }
  __syncthreads();          // every wave of this workgroup is past its last use of n
  if (threadIdx.x == 0) {
    const int drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn == (int)gridDim.x - 1) {
      __hip_atomic_store(n_averaged, n + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

int avg_flat_launch(float* avg, const float* p, int64_t begin, int64_t end, int kind, float w, int64_t* n_averaged,
                    int32_t* ticket, hipStream_t stream) {
  static const char* who = "avg flat";
  MFM_REQUIRE(avg && p && n_averaged && ticket, "%s: bad arguments (avg, p, n_averaged and ticket must not be null)", who);
  MFM_REQUIRE((((uintptr_t)avg | (uintptr_t)p) & 15) == 0, "%s: avg and p must be 16-byte aligned", who);
  MFM_REQUIRE(begin >= 0 && end > begin && (begin & 3) == 0 && (end & 3) == 0,
              "%s: [%lld,%lld) (bounds multiples of 4 elements, end above begin)", who, (long long)begin, (long long)end);
  MFM_REQUIRE(kind == MFM_AVG_SWA || kind == MFM_AVG_EMA, "%s: unknown kind %d", who, kind);
  MFM_REQUIRE(kind != MFM_AVG_EMA || (w >= 0.0f && w <= 1.0f), "%s: EMA weight %g (must be in [0, 1], not NaN)", who, (double)w);
  MFM_REQUIRE(((uintptr_t)n_averaged & 7) == 0 && ((uintptr_t)ticket & 3) == 0,
              "%s: n_averaged must be 8-byte aligned (an int64 word) and ticket 4-byte aligned", who);
  const int64_t b4 = begin >> 2, e4 = end >> 2;
  int32_t tiles;
  int nb;
  if (int rc = span_grid(who, (e4 - b4 + kSpanTile - 1) / kSpanTile, &tiles, &nb)) return rc;
  MFM_LAUNCH_TIMED(avg_flat_kernel, dim3(nb), dim3(kSpanTile), 0, stream, avg, p, b4, e4, (int)tiles, kind, w, n_averaged, ticket);
  MFM_LAUNCH_CHECK("avg_flat_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_avg_flat(float* avg, const float* p, int64_t begin, int64_t end, int32_t kind, float w, int64_t* n_averaged,
                            int32_t* ticket, void* stream) {
  return mfm::avg_flat_launch(avg, p, begin, end, kind, w, n_averaged, ticket, (hipStream_t)stream);
}
