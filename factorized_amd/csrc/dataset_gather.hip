// Per-epoch reshuffle of an HBM-resident split (factorized_amd.train.DeviceDataset.reshuffle): one launch gathers the samples of
// a sample-major pool X_pool [N, T, D] / y_pool [N, ybytes] through a device permutation into the batch layout the plans consume,
//   X[b, t, r, :] = X_pool[perm[b * B + r], t, :]      y[b, r, :] = y_pool[perm[b * B + r], :]      b < nb, t < T, r < B.
// A pure copy: the data only passes through registers, so every bit pattern (NaN payloads included) arrives unchanged.
//
// Work is dealt in destination rows q = (b * T + t) * B + r of D floats, one row per wave and turn: 256 threads = 4 rows per
// workgroup, at most 2048 workgroups grid-striding over the nb * T * B rows.  A destination row is contiguous and so is its
// source row, so a wave instruction moves 64 consecutive accesses (1 KiB with 16-byte accesses, 256 B with dwords).  All that
// depends on the row -- its (b, t, r), the sample index, both base addresses -- is wave-uniform and lives in SGPRs; a lane adds
// its column.  The wave that has a row of t == 0 also moves that sample's label row, with the index it already holds.
//
// Two dependent latencies per row (the index, then the row) are what a gather adds to a copy.  The index of a wave's NEXT row is
// requested before the current row moves, and up to kGatherInFlight accesses per lane are loaded before the first is stored,
// so that a wave keeps a whole canonical row (325 floats) in flight.
//
// 16-byte accesses need every row of both buffers 16-byte aligned: D % 4 == 0 and both bases aligned (the host picks the
// form).  Otherwise dwords: the canonical D = 325 leaves rows only 4-byte aligned, and source and destination rows then
// differ in their alignment, so no wider access fits both.  Labels always move as dwords.
//
// A sample index outside [0, N) is skipped: its destination rows keep their bytes, nothing is read.  (DeviceDataset validates
// a caller's permutation once, in Python; this is the bound that holds whatever arrives.)
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage):
//   dataset_gather_kernel<4>   VGPRs 36   AGPRs 0   SGPRs 52   scratch 0 bytes   LDS 0 bytes   occupancy 8 waves/SIMD
//   dataset_gather_kernel<1>   VGPRs 24   AGPRs 0   SGPRs 50   scratch 0 bytes   LDS 0 bytes   occupancy 8 waves/SIMD
// In the generated code the indices arrive by s_load_dwordx2, the rows move as global_load / global_store_dwordx4 (dword), the
// loads of a turn are issued before its first store, and there is no scalar-side or LDS traffic besides.
#include <type_traits>

#include "internal.h"

namespace mfm {

constexpr int kGatherThreads = 256;
constexpr int kGatherRowsPerWg = kGatherThreads / 64;      // one row per wave
constexpr int kGatherMaxWgs = 2048;
constexpr int kGatherInFlight = 4;                         // accesses per lane loaded before the first store

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One wave copies n consecutive accesses of type V (dst and src aligned to V).
template <class V>
__device__ __forceinline__ void gather_row(V* __restrict__ dst, const V* __restrict__ src, int n, int lane) {
  for (int c = lane; c < n; c += 64 * kGatherInFlight) {
    V v[kGatherInFlight];
#pragma unroll
    for (int u = 0; u < kGatherInFlight; ++u)
      if (c + 64 * u < n) v[u] = src[c + 64 * u];
#pragma unroll
    for (int u = 0; u < kGatherInFlight; ++u)
      if (c + 64 * u < n) dst[c + 64 * u] = v[u];
  }
}

// VEC: dwords per access of the X rows (4 or 1).  rows = nb * T * B <= INT32_MAX; yw = dwords per label row.
template <int VEC>
__global__ __launch_bounds__(kGatherThreads) void dataset_gather_kernel(uint32_t* __restrict__ X, uint32_t* __restrict__ y,
                                                                        const uint32_t* __restrict__ Xp,
                                                                        const uint32_t* __restrict__ yp,
                                                                        const int64_t* __restrict__ perm, int64_t N, uint32_t rows,
                                                                        uint32_t T, uint32_t B, uint32_t D, uint32_t yw) {
  typedef typename std::conditional<VEC == 4, u32x4, uint32_t>::type V;
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t stride = gridDim.x * kGatherRowsPerWg;          // rows + stride < 2^32: no wrap-around
  uint32_t q = blockIdx.x * kGatherRowsPerWg + wave;
  if (q >= rows) return;
  // position b * B + r of row q in the permutation
  auto slot = [&](uint32_t row) { const uint32_t bt = row / B; return (int64_t)(bt / T) * B + (row - bt * B); };
  int64_t s_next = perm[slot(q)];
  for (; q < rows; q += stride) {
    const int64_t s = s_next;
    if (q + stride < rows) s_next = perm[slot(q + stride)];
    if (s < 0 || s >= N) continue;
    const uint32_t bt = q / B, b = bt / T, t = bt - b * T, r = q - bt * B;
    gather_row<V>(reinterpret_cast<V*>(X + (int64_t)q * D), reinterpret_cast<const V*>(Xp + (s * T + t) * D), (int)(D / VEC), lane);
    if (t == 0) gather_row<uint32_t>(y + ((int64_t)b * B + r) * yw, yp + s * yw, (int)yw, lane);
  }
}

static bool ranges_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

int dataset_gather_launch(float* X, void* y, const float* X_pool, const void* y_pool, const int64_t* perm, int64_t N, int nb,
                          int T, int B, int D, int64_t ybytes, hipStream_t stream) {
  static const char* who = "dataset gather";
  MFM_REQUIRE(X && y && X_pool && y_pool && perm, "%s: bad arguments (X, y, X_pool, y_pool and perm must not be null)", who);
  MFM_REQUIRE(N >= 1 && nb >= 1 && T >= 1 && B >= 1 && D >= 1 && D <= (1 << 30),
              "%s: N %lld, nb %d, T %d, B %d, D %d (all must be positive, D at most 2^30)", who, (long long)N, nb, T, B, D);
  MFM_REQUIRE((int64_t)nb * B <= N, "%s: nb * B = %lld samples in the batches, N = %lld in the pool", who,
              (long long)((int64_t)nb * B), (long long)N);
  MFM_REQUIRE(ybytes >= 4 && (ybytes & 3) == 0 && ybytes <= INT32_MAX, "%s: ybytes %lld (a positive multiple of 4)", who,
              (long long)ybytes);
  const int64_t rows = (int64_t)nb * T * B;
  MFM_REQUIRE(rows <= INT32_MAX, "%s: nb * T * B = %lld rows (at most 2^31 - 1)", who, (long long)rows);
  MFM_REQUIRE(N <= INT64_MAX / 4 / T / D && N <= INT64_MAX / ybytes, "%s: pool of %lld samples too large", who, (long long)N);
  MFM_REQUIRE((((uintptr_t)X | (uintptr_t)X_pool | (uintptr_t)y | (uintptr_t)y_pool) & 3) == 0,
              "%s: X, y, X_pool and y_pool must be 4-byte aligned", who);
  MFM_REQUIRE(((uintptr_t)perm & 7) == 0, "%s: perm must be 8-byte aligned (int64 indices)", who);
  MFM_REQUIRE(!ranges_overlap(X, rows * D * 4, X_pool, N * T * D * 4) && !ranges_overlap(y, (int64_t)nb * B * ybytes, y_pool, N * ybytes),
              "%s: the batches and the pool must not overlap (the pool is the source of every reshuffle)", who);
  const bool vec = (D & 3) == 0 && (((uintptr_t)X | (uintptr_t)X_pool) & 15) == 0;
  const int64_t tiles = (rows + kGatherRowsPerWg - 1) / kGatherRowsPerWg;
  const dim3 grid((unsigned)(tiles < kGatherMaxWgs ? tiles : kGatherMaxWgs));
  uint32_t* Xd = reinterpret_cast<uint32_t*>(X);
  const uint32_t* Xs = reinterpret_cast<const uint32_t*>(X_pool);
  if (vec)
    MFM_LAUNCH_TIMED(dataset_gather_kernel<4>, grid, dim3(kGatherThreads), 0, stream, Xd, (uint32_t*)y, Xs, (const uint32_t*)y_pool,
                     perm, N, (uint32_t)rows, (uint32_t)T, (uint32_t)B, (uint32_t)D, (uint32_t)(ybytes >> 2));
  else
    MFM_LAUNCH_TIMED(dataset_gather_kernel<1>, grid, dim3(kGatherThreads), 0, stream, Xd, (uint32_t*)y, Xs, (const uint32_t*)y_pool,
                     perm, N, (uint32_t)rows, (uint32_t)T, (uint32_t)B, (uint32_t)D, (uint32_t)(ybytes >> 2));
  MFM_LAUNCH_CHECK("dataset_gather_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_dataset_gather(float* X, void* y, const float* X_pool, const void* y_pool, const int64_t* perm, int64_t N,
                                  int32_t nb, int32_t T, int32_t B, int32_t D, int64_t ybytes, void* stream) {
  return mfm::dataset_gather_launch(X, y, X_pool, y_pool, perm, N, nb, T, B, D, ybytes, (hipStream_t)stream);
}
